// csrc/eds_inisetup.hpp (namespace edsini: gridMaxSelection and makePixelStatus as the host restates them) and makeNN's tables
// (edsini::make_nn of csrc/eds_init.hpp over csrc/eds_nntree.hpp, nanoflann's build and walk) behind a C interface for ctypes.
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

// makeNN's tables with their squared distances and the two trees' depths; stack: the deepest tree the explicit walk takes (a deeper
// one is walked by recursion), 0 .. edsnn::STACK
int inisetup_make_nn(int n, const float* uv, int n_up, const float* uv_up, int stack, int32_t* nb, float* nb_dist, int32_t* parent,
                     float* parent_dist, int32_t* depth) {
    int d[2] = {0, 0};
    make_nn(n, uv, parent ? n_up : 0, uv_up, nb, parent, stack, nb_dist, parent_dist, d);
    if (depth) { depth[0] = d[0]; depth[1] = d[1]; }
    return 0;
}

int inisetup_make_nn_exhaustive(int n, const float* uv, int n_up, const float* uv_up, int32_t* nb, int32_t* parent) {
    make_nn_exhaustive(n, uv, parent ? n_up : 0, uv_up, nb, parent);
    return 0;
}

int inisetup_nn_stack(void) { return edsnn::STACK; }

// the build alone (what eds_ini_make_neighbours does on the host per level): returns the tree's depth
int inisetup_nn_build(int n, const float* uv) {
    edsnn::Tree t;
    edsnn::build(uv, n, t);
    return t.depth;
}

}  // extern "C"

#ifdef INISETUP_STANDALONE
namespace {
// makeNN over one cloud and a level above it, through the explicit walk and through the recursion: every index in range, the point
// itself among its neighbours where distances are finite, both walks the same.  Returns the number of table entries, -1 on a fault.
long nn_case(const std::vector<float>& uv, const std::vector<float>& up, bool finite) {
    const int n = (int)(uv.size() / 2), n_up = (int)(up.size() / 2);
    std::vector<int32_t> nb((size_t)n * NN + 1), par((size_t)n + 1), nb2(nb.size()), par2(par.size());
    std::vector<float> nd((size_t)n * NN + 1), pd((size_t)n + 1);
    int32_t depth[2];
    inisetup_make_nn(n, n ? uv.data() : nullptr, n_up, n_up ? up.data() : nullptr, edsnn::STACK, nb.data(), nd.data(), n_up ? par.data() : nullptr,
                     pd.data(), depth);
    inisetup_make_nn(n, n ? uv.data() : nullptr, n_up, n_up ? up.data() : nullptr, 0, nb2.data(), nullptr, n_up ? par2.data() : nullptr, nullptr,
                     nullptr);
    long entries = 0;
    for (int i = 0; i < n; ++i) {
        bool self = false;
        for (int k = 0; k < NN; ++k) {
            const int32_t j = nb[(size_t)i * NN + k];
            if (j < -1 || j >= n || j != nb2[(size_t)i * NN + k]) return -1;
            if (finite && (j >= 0) != (k < n)) return -1;
            if (k > 0 && j >= 0 && nd[(size_t)i * NN + k] < nd[(size_t)i * NN + k - 1]) return -1;
            self = self || j == i;
            entries += j >= 0;
        }
        if (finite && !self && nd[(size_t)i * NN + (n < NN ? n : NN) - 1] > 0.0f) return -1;
        if (n_up && (par[i] < 0 || par[i] >= n_up || par[i] != par2[i])) return -1;
    }
    return entries;
}
}  // namespace

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
    // makeNN: no points, one point, all points identical, collinear points, coordinates up to 8 191.1, a tree deeper than the walk's
    // stack, and coordinates that are not finite (refused by the C entry points; here they must only stay inside the arrays)
    {
        std::vector<std::vector<float>> clouds;
        clouds.push_back({});
        clouds.push_back({3.1f, 3.1f});
        clouds.push_back(std::vector<float>(2 * 37, 5.1f));
        { std::vector<float> c; for (int i = 0; i < 200; ++i) { c.push_back((float)(3 * i + 0.1)); c.push_back(7.1f); } clouds.push_back(c); }
        { std::vector<float> c; for (int i = 0; i < 150; ++i) { c.push_back(4.1f); c.push_back((float)(i + 0.1)); } clouds.push_back(c); }
        { std::vector<float> c; for (int i = 0; i < 600; ++i) { c.push_back((float)((int)(8191 * rnd()) + 0.1)); c.push_back((float)((int)(8191 * rnd()) + 0.1)); }
          c.push_back(8191.1f); c.push_back(8191.1f); c.push_back(0.1f); c.push_back(8191.1f); clouds.push_back(c); }
        { std::vector<float> c; for (int i = 0; i < 40 * 32; ++i) if (i % 3 == 0) { c.push_back((float)(i % 40 + 0.1)); c.push_back((float)(i / 40 + 0.1)); } clouds.push_back(c); }
        { std::vector<float> c; float x = ldexpf(1.0f, -60); for (int i = 0; i < 120; ++i) { c.push_back(x); c.push_back(0.0f); x *= 2.0f; } clouds.push_back(c); }    // depth > STACK
        const size_t n_finite = clouds.size();
        { std::vector<float> c; for (int i = 0; i < 64; ++i) { c.push_back(100.0f * rnd()); c.push_back(100.0f * rnd()); }
          c[6] = NAN; c[21] = INFINITY; c[40] = -INFINITY; c[41] = NAN; c[90] = 3.0e38f; c[91] = -3.0e38f; clouds.push_back(c); }
        clouds.push_back(std::vector<float>(2 * 20, NAN));
        for (size_t a = 0; a < clouds.size(); ++a)
            for (size_t b = 0; b < clouds.size(); ++b) {
                const long e = nn_case(clouds[a], clouds[b], a < n_finite && b < n_finite);
                if (e < 0) { printf("inisetup standalone: makeNN failed on clouds %zu, %zu\n", a, b); return 2; }
                total += e;
                ++calls;
            }
    }
    printf("inisetup standalone: %ld calls, %ld points\n", calls, total);
    return 0;
}
#endif
