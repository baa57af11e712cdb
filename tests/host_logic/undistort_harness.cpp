// csrc/eds_undistort.hpp on the CPU: the entry points tests/undistort_harness.py binds.  The set-up half of that header is the very text
// eds_und_create and eds_und_set_photometric run inside the library; process_host is the reference's two passes over the per-pixel
// functions the kernels call.  Built with g++ -ffp-contract=off.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../slam-eds_amd/csrc/eds_undistort.hpp"

using namespace edsund;

struct Host {
    Setup s;
    bool passthrough = false;
    Photometric ph;
    Settings st = settings_default();
};

extern "C" {

int und_geometry_size(void) { return (int)sizeof(Geometry); }
int und_settings_size(void) { return (int)sizeof(Settings); }
void und_settings_default(Settings* s) { *s = settings_default(); }

// NULL with *rc = RC_INVALID or RC_NOT_USABLE; iterations (may be NULL) is filled either way
Host* und_new(const Geometry* g, int* rc, int* iterations) {
    Host* h = new Host;
    *rc = setup(*g, h->s);
    if (iterations) *iterations = h->s.iterations;
    if (*rc != RC_OK) { delete h; return nullptr; }
    h->passthrough = h->s.passthrough;
    return h;
}
void und_free(Host* h) { delete h; }
void und_get_K(const Host* h, double* K) { memcpy(K, h->s.K, sizeof(h->s.K)); }
void und_get_pars(const Host* h, double* pars) { memcpy(pars, h->s.g.pars, sizeof(h->s.g.pars)); }
void und_get_map(const Host* h, float* mapx, float* mapy) {
    memcpy(mapx, h->s.mapx.data(), h->s.mapx.size() * sizeof(float));
    memcpy(mapy, h->s.mapy.data(), h->s.mapy.size() * sizeof(float));
}
// out: passthrough, relative, iterations, shrinks[4], rule_pixels; range: minX, maxX, minY, maxY after the 1.01 widening
void und_info(const Host* h, int64_t* out, float* range) {
    out[0] = h->passthrough; out[1] = h->s.relative; out[2] = h->s.iterations;
    for (int i = 0; i < 4; ++i) { out[3 + i] = h->s.shrinks[i]; range[i] = h->s.range[i]; }
    out[7] = h->s.rule_pixels;
}
int und_set_map(Host* h, const float* mapx, const float* mapy) {
    const size_t n = (size_t)h->s.g.w * h->s.g.h;
    if (!map_valid(mapx, mapy, n, h->s.g.w_org, h->s.g.h_org)) return RC_INVALID;
    h->s.mapx.assign(mapx, mapx + n);
    h->s.mapy.assign(mapy, mapy + n);
    h->passthrough = false;
    return RC_OK;
}
int und_set_photometric(Host* h, const float* G, int g_depth, const void* vignette, int vignette_type) {
    return set_photometric(h->ph, G, g_depth, vignette, vignette_type, (size_t)h->s.g.w_org * h->s.g.h_org, h->st.photometric_calibration);
}
int und_set_settings(Host* h, const Settings* s) {
    if (!settings_valid(*s)) return RC_INVALID;
    h->st = *s;
    apply_mode_to_G(h->ph, s->photometric_calibration);
    return RC_OK;
}
// G: g_depth floats, vinv: w_org * h_org floats; returns g_depth, 0 without a calibration
int und_get_photometric(const Host* h, float* G, float* vinv) {
    if (!h->ph.valid) return 0;
    if (G) memcpy(G, h->ph.G.data(), h->ph.G.size() * sizeof(float));
    if (vinv) memcpy(vinv, h->ph.vignetteMapInv.data(), h->ph.vignetteMapInv.size() * sizeof(float));
    return h->ph.g_depth;
}
// one frame; out: w * h floats
int und_process(Host* h, const void* raw, int raw_type, int64_t row_stride, float exposure, float factor, float* out, float* exposure_out) {
    if (!raw_type_fits(h->ph, h->st.photometric_calibration, raw_type)) return RC_INVALID;
    Setup& s = h->s;
    const bool keep = s.passthrough;
    s.passthrough = h->passthrough;
    std::vector<float> plane((size_t)s.g.w_org * s.g.h_org);
    if (row_stride == 0) row_stride = s.g.w_org;
    const float e = raw_type == RAW_U16
                        ? process_host(s, h->ph, h->st, static_cast<const uint16_t*>(raw), row_stride, exposure, factor, plane.data(), out)
                        : process_host(s, h->ph, h->st, static_cast<const uint8_t*>(raw), row_stride, exposure, factor, plane.data(), out);
    s.passthrough = keep;
    if (exposure_out) *exposure_out = e;
    return RC_OK;
}

}  // extern "C"
