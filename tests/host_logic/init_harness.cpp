// csrc/eds_init.hpp (namespace edsini, what the device kernels run) under g++: a host handle with the entry points of
// include/eds_hip_init.h that runs edsini::track_frame over SerialEv, and the single steps the oracle tests compare one by one.
// Loaded through tests/init_harness.py; -DINI_STANDALONE makes the program of the sanitizer run (its own main, its own inputs).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../slam-eds_amd/csrc/eds_init.hpp"

using namespace edsini;

namespace {

struct HostIni {
    int cap = 0;
    Geo geo;
    Params prm;
    float exposure_first = 1.0f;
    Carry carry;
    std::vector<Px> first_px, new_px;
    std::vector<Pnt> pts;
    std::vector<int32_t> sched, parent, doff, coff, child, good_old;
    std::vector<float> jb, iR_old;
    int32_t n[MAX_LEVELS] = {0, 0, 0, 0, 0}, nd[MAX_LEVELS] = {0, 0, 0, 0, 0};
    Shared sh;
};

Frame make_frame(HostIni* h, const float* img) {
    Frame f;
    memset(&f, 0, sizeof(f));
    f.g = h->geo; f.s = h->prm;
    for (int l = 0; l < h->geo.levels; ++l) {
        const size_t o = (size_t)l * h->cap, o1 = (size_t)l * (h->cap + 1);
        Lv& L = f.lv[l];
        L.p = h->pts.data() + o; L.sched = h->sched.data() + o * SCHED; L.parent = h->parent.data() + o;
        L.doff = h->doff.data() + o1; L.coff = h->coff.data() + o1; L.child = h->child.data() + o; L.jb = h->jb.data() + o * 2 * 10;
        L.n = h->n[l]; L.nd = h->nd[l]; L.n_parents = l + 1 < h->geo.levels ? h->n[l + 1] : 0; L.cap = h->cap;
    }
    f.ref = h->first_px.data(); f.nw = h->new_px.data(); f.img = img; f.iR_old = h->iR_old.data(); f.good_old = h->good_old.data();
    return f;
}

void set_pose(HostIni* h, int which, const double* T, const double* aff) {
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) h->sh.R[which][3 * i + j] = T[4 * i + j];
        h->sh.t[which][i] = T[4 * i + 3];
    }
    h->sh.ab[which][0] = aff[0]; h->sh.ab[which][1] = aff[1];
}

}  // namespace

extern "C" {

int ini_sizes(int* pnt, int* result, int* sys) { *pnt = (int)sizeof(Pnt); *result = (int)sizeof(Result); *sys = (int)sizeof(Sys); return LANES; }
int ini_atan_max_ulp() { return edsct::ATAN_MAX_ULP; }
void ini_atan_n(const double* x, int n, double* out) { for (int i = 0; i < n; ++i) out[i] = edsct::atan_d(x[i]); }
void ini_log_upsilon(const double* T, double* ups) {
    double R[9], t[3];
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) R[3 * i + j] = T[4 * i + j]; t[i] = T[4 * i + 3]; }
    se3_log_upsilon(R, t, ups);
}
void ini_params_default(Params* p) { *p = params_default(); }

void* ini_create(int H, int W, int levels, int cap) {
    if (!edsct::shape_valid(H, W, levels) || cap < 1) return nullptr;
    HostIni* h = new HostIni;
    h->cap = cap;
    edsct::make_shape(h->geo, H, W, levels);
    h->prm = params_default();
    memset(&h->carry, 0, sizeof(h->carry));
    memset(&h->sh, 0, sizeof(h->sh));
    const size_t lc = (size_t)levels * cap;
    h->first_px.assign(h->geo.total, Px{0, 0, 0, 0}); h->new_px = h->first_px;
    Pnt zero;
    memset(&zero, 0, sizeof(zero));
    h->pts.assign(lc, zero);
    h->sched.assign(lc * SCHED, -1); h->parent.assign(lc, 0); h->doff.assign(lc + levels, 0); h->coff.assign(lc + levels, 0);
    h->child.assign(lc, 0); h->jb.assign(lc * 20, 0.0f); h->iR_old.assign(cap, 0.0f); h->good_old.assign(cap, 0);
    return h;
}
void ini_destroy(void* p) { delete (HostIni*)p; }
int ini_set_params(void* p, const Params* s) { if (!params_valid(*s)) return -1; ((HostIni*)p)->prm = *s; return 0; }
void ini_set_calib(void* p, float fx, float fy, float cx, float cy) { edsct::make_k(((HostIni*)p)->geo, fx, fy, cx, cy); }

void ini_set_first(void* p, const float* img, float exposure) {
    HostIni* h = (HostIni*)p;
    SerialEv ev;
    build_pyramid(ev, h->geo, img, h->first_px.data());
    const double aff[2] = {h->carry.aff[0], h->carry.aff[1]};
    memset(&h->carry, 0, sizeof(h->carry));
    h->carry.T[0] = h->carry.T[5] = h->carry.T[10] = 1.0;
    h->carry.aff[0] = aff[0]; h->carry.aff[1] = aff[1];
    h->exposure_first = exposure;
}

void ini_set_pose(void* p, const double* T, const double* aff) {
    HostIni* h = (HostIni*)p;
    memcpy(h->carry.T, T, sizeof(h->carry.T));
    h->carry.aff[0] = aff[0]; h->carry.aff[1] = aff[1];
}

int ini_set_points(void* p, int lvl, const float* status) {
    HostIni* h = (HostIni*)p;
    const Level& L = h->geo.l[lvl];
    int n = 0;
    for (int y = 0; y < L.h; ++y)
        for (int x = 0; x < L.w; ++x)
            if (in_rect(x, y, L.w, L.h) && status[x + y * L.w] != 0) {
                if (n < h->cap) h->pts[(size_t)lvl * h->cap + n] = make_point(x, y, status[x + y * L.w], h->prm);
                ++n;
            }
    for (size_t i = 0; i < (size_t)h->cap * 20; ++i) h->jb[(size_t)lvl * h->cap * 20 + i] = 0.0f;
    h->n[lvl] = n <= h->cap ? n : 0;
    return n;
}

int ini_make_nn(int n, const float* uv, int n_up, const float* uv_up, int32_t* nb, int32_t* parent) {
    make_nn(n, uv, parent ? n_up : 0, uv_up, nb, parent);
    return 0;
}

int ini_set_neighbours(void* p, int lvl, const int32_t* nb, const int32_t* parent) {
    HostIni* h = (HostIni*)p;
    const bool top = lvl == h->geo.levels - 1;
    const int n = h->n[lvl], np = top ? 0 : h->n[lvl + 1];
    const size_t o = (size_t)lvl * h->cap, o1 = (size_t)lvl * (h->cap + 1);
    std::vector<int32_t> sched(((size_t)n + 1) * SCHED), doff((size_t)n + 2), coff((size_t)np + 2), child((size_t)n + 1);
    int32_t nd = 0;
    if (!derive_tables(n, nb, top ? nullptr : parent, np, sched.data(), doff.data(), &nd, coff.data(), child.data())) return -1;
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < SCHED; ++j) h->sched[(o + i) * SCHED + j] = sched[(size_t)i * SCHED + j];
        if (!top) { h->parent[o + i] = parent[i]; h->child[o + i] = child[i]; }
    }
    for (int d = 0; d <= nd; ++d) h->doff[o1 + d] = doff[d];
    for (int k = 0; !top && k <= np; ++k) h->coff[o1 + k] = coff[k];
    h->nd[lvl] = nd;
    return 0;
}
int ini_schedule_depth(void* p, int lvl) { return ((HostIni*)p)->nd[lvl]; }

void ini_track_frame(void* p, const float* img, float exposure, int snapped_threshold, Result* out) {
    HostIni* h = (HostIni*)p;
    Frame f = make_frame(h, img);
    f.have_guess = (h->exposure_first > 0 && exposure > 0) ? 1 : 0;
    f.aff_guess = f.have_guess ? logf(exposure / h->exposure_first) : 0.0f;
    f.snapped_threshold = snapped_threshold;
    memset(out, 0, sizeof(*out));
    SerialEv ev;
    track_frame(ev, f, &h->sh, &h->carry, out);
    out->launches = 1; out->waits = 1;
}

int ini_get_points(void* p, int lvl, Pnt* out) {
    HostIni* h = (HostIni*)p;
    for (int i = 0; i < h->n[lvl]; ++i) out[i] = h->pts[(size_t)lvl * h->cap + i];
    return h->n[lvl];
}
void ini_set_points_state(void* p, int lvl, const Pnt* in) {
    HostIni* h = (HostIni*)p;
    for (int i = 0; i < h->n[lvl]; ++i) h->pts[(size_t)lvl * h->cap + i] = in[i];
}
void ini_get_jb(void* p, int lvl, int which, float* out) {
    HostIni* h = (HostIni*)p;
    const int idx = which == 0 ? h->carry.jb_cur[lvl] : 1 - h->carry.jb_cur[lvl];
    memcpy(out, h->jb.data() + ((size_t)lvl * 2 + idx) * h->cap * 10, (size_t)h->n[lvl] * 10 * sizeof(float));
}
void ini_set_jb(void* p, int lvl, int which, const float* in) {
    HostIni* h = (HostIni*)p;
    const int idx = which == 0 ? h->carry.jb_cur[lvl] : 1 - h->carry.jb_cur[lvl];
    memcpy(h->jb.data() + ((size_t)lvl * 2 + idx) * h->cap * 10, in, (size_t)h->n[lvl] * 10 * sizeof(float));
}
void ini_get_level(void* p, int which, int lvl, float* out) {
    HostIni* h = (HostIni*)p;
    const Level& L = h->geo.l[lvl];
    const Px* px = (which == 0 ? h->first_px.data() : h->new_px.data()) + L.off;
    for (int i = 0; i < L.w * L.h; ++i) { out[3 * i] = px[i].c; out[3 * i + 1] = px[i].dx; out[3 * i + 2] = px[i].dy; }
}
void ini_set_new(void* p, const float* img) {
    HostIni* h = (HostIni*)p;
    SerialEv ev;
    build_pyramid(ev, h->geo, img, h->new_px.data());
}
void ini_get_carry(void* p, Carry* out) { *out = ((HostIni*)p)->carry; }

// ---- the single steps, on the state the handle holds ------------------------------------------------------------------------------------
// the first loop of calcResAndGS at pose (T, aff): the rows before the alphaOpt terms, residual and hw per tap (n x 8 x 2, untouched
// where a tap was not reached), the 46 sums; the points' maxstep, energy_new and isGood_new change as the loop changes them
void ini_first_loop(void* p, int lvl, const double* T, const double* aff, float* rows, float* taps, double* sums) {
    HostIni* h = (HostIni*)p;
    Frame f = make_frame(h, nullptr);
    set_pose(h, 0, T, aff);
    const Warp w = make_warp(f.g, lvl, f.s, h->sh.R[0], h->sh.t[0], aff[0], aff[1]);
    const Lv& L = f.lv[lvl];
    const Px *ref = f.ref + f.g.l[lvl].off, *nw = f.nw + f.g.l[lvl].off;
    SerialEv ev;
    ev.reduce<46>(L.n, sums, [&](int i, double* acc) { point_calc(w, ref, nw, L.p[i], rows + (size_t)i * 10, acc, taps + (size_t)i * 16); });
}
// the whole of calcResAndGS into JbBuffer_new; sc_sums: the 45 fp64 sums of acc9SC
void ini_calc(void* p, int lvl, const double* T, const double* aff, Sys* out, double* sc_sums) {
    HostIni* h = (HostIni*)p;
    Frame f = make_frame(h, nullptr);
    set_pose(h, 0, T, aff);
    SerialEv ev;
    calc(ev, f, &h->sh, lvl, 0, f.lv[lvl].jb + (size_t)(1 - h->carry.jb_cur[lvl]) * h->cap * 10);
    *out = h->sh.sys[0];
    for (int q = 0; q < 45; ++q) sc_sums[q] = h->sh.S[q];          // the last reduce of calc is acc9SC's
}
void ini_calc_ec(void* p, int lvl, int snapped, float* out) {
    HostIni* h = (HostIni*)p;
    Frame f = make_frame(h, nullptr);
    SerialEv ev;
    calc_ec(ev, f, &h->sh, lvl, snapped, out);
}
void ini_do_step(void* p, int lvl, float lambda, const float* inc) {
    HostIni* h = (HostIni*)p;
    Frame f = make_frame(h, nullptr);
    SerialEv ev;
    do_step(ev, f, lvl, lambda, inc, f.lv[lvl].jb + (size_t)h->carry.jb_cur[lvl] * h->cap * 10);
}
void ini_apply_step(void* p, int lvl) {
    HostIni* h = (HostIni*)p;
    Frame f = make_frame(h, nullptr);
    SerialEv ev;
    apply_step(ev, f, lvl);
    h->carry.jb_cur[lvl] ^= 1;
}
void ini_opt_reg(void* p, int lvl, int snapped) { HostIni* h = (HostIni*)p; Frame f = make_frame(h, nullptr); SerialEv ev; opt_reg(ev, f, lvl, snapped); }
void ini_reset_points(void* p, int lvl) { HostIni* h = (HostIni*)p; Frame f = make_frame(h, nullptr); SerialEv ev; reset_points(ev, f, lvl); }
void ini_propagate_down(void* p, int src, int snapped) { HostIni* h = (HostIni*)p; Frame f = make_frame(h, nullptr); SerialEv ev; propagate_down(ev, f, src, snapped); }
void ini_propagate_up(void* p, int src, int snapped) { HostIni* h = (HostIni*)p; Frame f = make_frame(h, nullptr); SerialEv ev; propagate_up(ev, f, src, snapped); }
void ini_solve_inc(const Sys* y, const Params* s, float lambda, int wh, float* inc) { solve_inc(*y, *s, lambda, wh, inc); }

}  // extern "C"

#ifdef INI_STANDALONE
// The program of the sanitizer run: a textured pair of its own, full-density status maps, exact tables, six frames; then hostile inputs
// (NaN / inf images and exposures, an empty level, tables full of -1).  Prints one line.
static float tex(double x, double y) { return (float)(128.0 + 45.0 * sin(0.21 * x + 0.09 * y) + 35.0 * cos(0.12 * y - 0.05 * x) + 9.0 * sin(0.5 * x - 0.37 * y)); }

int main() {
    const int H = 48, W = 64, levels = 3, cap = 4096;
    long tracks = 0, iters = 0, points = 0;
    for (int variant = 0; variant < 4; ++variant) {
        void* h = ini_create(H, W, levels, cap);
        if (!h) return 2;
        ini_set_calib(h, 58.0f, 61.5f, 30.3f, 25.1f);
        std::vector<float> img((size_t)H * W);
        for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) img[x + y * W] = tex(x, y);
        ini_set_first(h, img.data(), variant == 2 ? NAN : 1.0f);
        std::vector<std::vector<float>> uv(levels);
        for (int l = 0; l < levels; ++l) {
            const int w = W >> l, hh = H >> l;
            std::vector<float> status((size_t)w * hh, 0.0f);
            for (int i = 0; i < w * hh; ++i) status[i] = (variant == 3 && l == 1) ? 0.0f : ((l == 0 && i % 3) ? 0.0f : 1.0f);
            const int n = ini_set_points(h, l, status.data());
            std::vector<Pnt> pts((size_t)n + 1);
            ini_get_points(h, l, pts.data());
            for (int i = 0; i < n; ++i) { uv[l].push_back(pts[i].u); uv[l].push_back(pts[i].v); }
            points += n;
        }
        for (int l = 0; l < levels; ++l) {
            const int n = (int)uv[l].size() / 2, nu = l + 1 < levels ? (int)uv[l + 1].size() / 2 : 0;
            std::vector<int32_t> nb((size_t)n * NN + 1, -1), par((size_t)n + 1, 0);
            if (nu > 0 || l + 1 == levels) ini_make_nn(n, uv[l].data(), nu, nu ? uv[l + 1].data() : nullptr, nb.data(), nu ? par.data() : nullptr);
            if (variant == 1) for (size_t i = 0; i < nb.size(); i += 3) nb[i] = -1;
            if (l + 1 < levels && nu == 0) { ini_destroy(h); h = nullptr; break; }      // no parents: the API refuses such tables
            if (ini_set_neighbours(h, l, nb.data(), l + 1 < levels ? par.data() : nullptr)) return 3;
        }
        if (!h) continue;
        for (int k = 1; k <= 6; ++k) {
            for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) img[x + y * W] = tex(x + 0.35 * k, y - 0.2 * k);
            if (variant == 2 && k == 3) img[100] = NAN;
            if (variant == 2 && k == 4) img[200] = INFINITY;
            Result r;
            ini_track_frame(h, img.data(), variant == 2 && k == 5 ? -1.0f : 1.0f, 1, &r);
            ++tracks;
            for (int l = 0; l < levels; ++l) iters += r.iters[l];
        }
        ini_destroy(h);
    }
    printf("init standalone: %ld tracks, %ld iterations, %ld points\n", tracks, iters, points);
    return 0;
}
#endif
