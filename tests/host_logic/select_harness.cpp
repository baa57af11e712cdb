// csrc/eds_pixsel.hpp on the CPU: the entry points tests/select_harness.py binds, and — with -DSEL_STANDALONE — a program of its own
// that runs a dumped set of cases plus hostile inputs (for a sanitizer build; it is never loaded into python that way).
// Built with g++ -ffp-contract=off.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../slam-eds_amd/csrc/eds_pixsel.hpp"

using namespace edspix;

extern "C" {

int sel_params_size(void) { return (int)sizeof(Params); }
int sel_pass_size(void) { return (int)sizeof(Pass); }
void sel_params_default(Params* p) { *p = params_default(); }
int sel_params_valid(const Params* p) { return params_valid(*p) ? 1 : 0; }
void sel_fill_reference_pattern(uint8_t* out, size_t n) { fill_reference_pattern(out, n); }

Serial* sel_new(int H, int W) {
    Serial* s = new Serial;
    serial_init(*s, H, W);
    return s;
}
void sel_free(Serial* s) { delete s; }
void sel_set_params(Serial* s, const Params* p) { s->prm = *p; s->hist_valid = false; }
void sel_set_table(Serial* s, const uint8_t* t, size_t n) { s->table.assign(t, t + n); }
void sel_set_potential(Serial* s, int p) { s->potential = p; }
int sel_get_potential(const Serial* s) { return s->potential; }
int sel_hist_valid(const Serial* s) { return s->hist_valid ? 1 : 0; }
void sel_set_image(Serial* s, const float* image, int64_t row_stride, const float* B) { serial_set_image(*s, image, row_stride, B); }

// passes: max_passes entries; pass_maps: max_passes x H x W bytes or NULL; returns numHaveSub
int sel_make_maps(Serial* s, float density, int recursions_left, float th_factor, Pass* passes, int max_passes, int* n_passes, uint8_t* pass_maps) {
    std::vector<Pass> ps;
    std::vector<std::vector<uint8_t>> maps;
    const int r = make_maps_serial(*s, density, recursions_left, th_factor, &ps, pass_maps ? &maps : nullptr);
    for (size_t i = 0; i < ps.size() && (int)i < max_passes; ++i) {
        passes[i] = ps[i];
        if (pass_maps) memcpy(pass_maps + i * s->map.size(), maps[i].data(), s->map.size());
    }
    if (n_passes) *n_passes = (int)ps.size();
    return r;
}
void sel_get_map(const Serial* s, uint8_t* out) { memcpy(out, s->map.data(), s->map.size()); }
void sel_get_level(const Serial* s, int lvl, float* out) { memcpy(out, s->lv[lvl].data(), s->lv[lvl].size() * sizeof(Px)); }
void sel_get_thresholds(const Serial* s, int smoothed, float* out) {
    const std::vector<float>& t = smoothed ? s->ths_s : s->ths;
    memcpy(out, t.data(), t.size() * sizeof(float));
}
void sel_scan_info(const Serial* s, int* ambiguous, int* n2_certain) { *ambiguous = s->ambiguous; *n2_certain = s->n2_certain; }
// uv: H * W * 2 ints, type: H * W floats at the most
int sel_selection(const Serial* s, int32_t* uv, float* type) {
    std::vector<int32_t> u;
    std::vector<float> t;
    const int n = selection_serial(*s, u, t);
    if (n > 0 && uv) memcpy(uv, u.data(), u.size() * sizeof(int32_t));
    if (n > 0 && type) memcpy(type, t.data(), t.size() * sizeof(float));
    return n;
}

}  // extern "C"

#ifdef SEL_STANDALONE
namespace {

struct Case {
    int H, W, potential, recursions, has_B;
    Params prm;
    float density, thf;
    std::vector<float> image, B;
    std::vector<uint8_t> table;
};

bool rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

long g_runs = 0, g_selected = 0;

void run(const Case& c) {
    Serial s;
    serial_init(s, c.H, c.W);
    s.prm = c.prm;
    s.table = c.table;
    s.potential = c.potential;
    serial_set_image(s, c.image.data(), c.W, c.has_B ? c.B.data() : nullptr);
    std::vector<Pass> ps;
    const int n = make_maps_serial(s, c.density, c.recursions, c.thf, &ps, nullptr);
    std::vector<int32_t> uv;
    std::vector<float> ty;
    if (selection_serial(s, uv, ty) != n) { printf("selection list and numHaveSub differ\n"); exit(3); }
    // a second call on the same image: the histograms are kept
    make_maps_serial(s, c.density, c.recursions, c.thf, nullptr, nullptr);
    ++g_runs;
    g_selected += n;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: %s cases.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    int32_t n_cases = 0;
    if (!rd(f, &n_cases, 4)) return 2;
    std::vector<Case> cases((size_t)n_cases);
    for (Case& c : cases) {
        int32_t hd[5];
        if (!rd(f, hd, sizeof(hd)) || !rd(f, &c.prm, sizeof(Params)) || !rd(f, &c.density, 4) || !rd(f, &c.thf, 4)) return 2;
        c.H = hd[0]; c.W = hd[1]; c.potential = hd[2]; c.recursions = hd[3]; c.has_B = hd[4];
        c.image.resize((size_t)c.H * c.W); c.table.resize((size_t)c.H * c.W); c.B.resize(256);
        if (!rd(f, c.image.data(), c.image.size() * 4) || !rd(f, c.table.data(), c.table.size()) || !rd(f, c.B.data(), 256 * 4)) return 2;
    }
    fclose(f);
    for (const Case& c : cases) run(c);
    const long committed = g_runs;

    // hostile inputs over the first case's shape and a 32 x 32 image
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    long hostile = 0;
    for (int shape = 0; shape < 2; ++shape) {
        Case b = cases[0];
        if (shape == 1) {
            b.H = 32; b.W = 32;
            b.image.assign(32 * 32, 0.0f);
            for (int i = 0; i < 32 * 32; ++i) b.image[i] = (float)((i * 37) % 251);
            b.table.assign(32 * 32, 0);
            for (int i = 0; i < 32 * 32; ++i) b.table[i] = (uint8_t)(i * 13);
        }
        const float bad[4] = {nan, inf, -inf, 1e30f};
        for (int k = 0; k < 4; ++k)                       // NaN, +-inf and 1e30 pixels: scattered, then everywhere
            for (int every = 0; every < 2; ++every) {
                Case c = b;
                for (size_t i = 0; i < c.image.size(); ++i)
                    if (every || i % 7 == 3) c.image[i] = bad[k];
                for (int withB = 0; withB < 2; ++withB) { c.has_B = withB; run(c); ++hostile; }
            }
        { Case c = b; c.has_B = 1; c.B.assign(256, 0.0f); run(c); ++hostile; }                 // a B table of zeros
        { Case c = b; c.table.assign(c.table.size(), 255); run(c); ++hostile; }               // an all-255 and an all-0 random table
        { Case c = b; c.table.assign(c.table.size(), 0); run(c); ++hostile; }
        const float dens[2] = {1.0f, (float)(b.W * b.H)};
        for (float d : dens)
            for (int rec = 0; rec < 4; rec += 3) { Case c = b; c.density = d; c.recursions = rec; run(c); ++hostile; }
        const int pots[2] = {1, 10000};
        for (int p : pots)
            for (int rec = 0; rec < 3; rec += 2) { Case c = b; c.potential = p; c.recursions = rec; run(c); ++hostile; }
        const float thfs[2] = {1e-30f, 1e30f};
        for (float t : thfs) { Case c = b; c.thf = t; c.recursions = 2; run(c); ++hostile; }
        { Case c = b; c.potential = MAX_POTENTIAL; c.density = 1e-30f; c.recursions = 3; run(c); ++hostile; }
        { Case c = b; c.prm.min_grad_hist_cut = 1.0f; run(c); ++hostile; }                    // the quantile walks past bin 49
        { Case c = b; c.prm.min_grad_hist_cut = 0.0f; c.prm.min_grad_hist_add = -1e30f; run(c); ++hostile; }
    }
    printf("select: %ld committed cases, %ld hostile inputs, %ld runs, %ld pixels selected\n", committed, hostile, g_runs, g_selected);
    return 0;
}
#endif
