// csrc/eds_coarse.hpp on the CPU: a host object with the entry points of include/eds_hip_coarse.h that tests/coarse_harness.py binds,
// and — with -DCT_STANDALONE — a program of its own that runs a dumped set of cases plus hostile inputs (for a sanitizer build; it is
// never loaded into python that way).  Built with g++ -ffp-contract=off.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../slam-eds_amd/csrc/eds_coarse.hpp"

using namespace edsct;

static_assert(sizeof(Term) == 64, "the python side reads a row as 16 words");
static_assert(sizeof(TrackOut) == 744, "the python side reads a result as eds_ct_result");

struct HostCt {
    Geo g;
    Params s;
    Photo ph;
    std::vector<Px> ref, nw;
    std::vector<float> idepth, wsum;
    std::vector<Pc> pc;
    int32_t pc_n[MAX_LEVELS];
};

static SerialEval evaluator(const HostCt* h) {
    SerialEval ev;
    ev.g = &h->g; ev.s = h->s; ev.ph = h->ph; ev.new_px = h->nw.data(); ev.pc = h->pc.data(); ev.pc_n = h->pc_n;
    ev.n_warped = 0;
    return ev;
}

extern "C" {

int ct_sizes(int* term, int* track_out) { *term = (int)sizeof(Term); *track_out = (int)sizeof(TrackOut); return LANES; }
void ct_ulp_bounds(int* sincos, int* exp) { *sincos = SINCOS_MAX_ULP; *exp = EXP_MAX_ULP; }
int ct_shape_valid(int H, int W, int levels) { return shape_valid(H, W, levels) ? 1 : 0; }
void ct_sincos_n(const double* x, int n, double* s, double* c) { for (int i = 0; i < n; ++i) sincos_d(x[i], s + i, c + i); }
void ct_exp_n(const double* x, int n, double* e) { for (int i = 0; i < n; ++i) e[i] = exp_d(x[i]); }

HostCt* ct_create(int H, int W, int levels) {
    if (!shape_valid(H, W, levels)) return nullptr;
    HostCt* h = new HostCt;
    make_shape(h->g, H, W, levels);
    h->s = params_default();
    h->ph.exposure_ref = h->ph.exposure_new = 1.0f; h->ph.ref_a = h->ph.ref_b = 0.0;
    const Px zero = {0.0f, 0.0f, 0.0f, 0.0f};
    const Pc none = {0.0f, 0.0f, 0.0f, 0.0f};
    h->ref.assign((size_t)h->g.total, zero); h->nw.assign((size_t)h->g.total, zero);
    h->idepth.assign((size_t)h->g.total, 0.0f); h->wsum.assign((size_t)h->g.total, 0.0f);
    h->pc.assign((size_t)h->g.total, none);
    for (int l = 0; l < MAX_LEVELS; ++l) h->pc_n[l] = 0;
    return h;
}
void ct_destroy(HostCt* h) { delete h; }
void ct_set_params(HostCt* h, const Params* p) { h->s = *p; }
void ct_set_calib(HostCt* h, float fx, float fy, float cx, float cy) { make_k(h->g, fx, fy, cx, cy); }
void ct_get_k(const HostCt* h, int lvl, float* K) { const Level& L = h->g.l[lvl]; K[0] = L.fx; K[1] = L.fy; K[2] = L.cx; K[3] = L.cy; }

int ct_set_ref(HostCt* h, const float* image, float exposure, double a, double b, int n, const float* cp, const float* hdif, int32_t* pc_n_out) {
    make_pyramid(h->g, image, h->g.W, h->ref.data());
    const int dropped = make_depth(h->g, h->ref.data(), n, cp, hdif, h->idepth.data(), h->wsum.data(), h->pc.data(), h->pc_n);
    h->ph.exposure_ref = exposure; h->ph.ref_a = a; h->ph.ref_b = b;
    if (pc_n_out) for (int l = 0; l < h->g.levels; ++l) pc_n_out[l] = h->pc_n[l];
    return dropped;
}
void ct_set_new(HostCt* h, const float* image, float exposure) {
    make_pyramid(h->g, image, h->g.W, h->nw.data());
    h->ph.exposure_new = exposure;
}

void ct_track(const HostCt* h, int count, const double* T, const double* aff, int coarsest, const double* min_res, TrackOut* out) {
    SerialEval ev = evaluator(h);
    for (int k = 0; k < count; ++k) track_serial(ev, T + 12 * k, aff + 2 * k, coarsest, min_res, out + k);
}

void ct_calc_res(const HostCt* h, int lvl, const double* T, const double* aff, float cutoff, double* rs, double* H, double* b, Term* rows) {
    SerialEval ev = evaluator(h);
    double R[9], t[3];
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) R[3 * i + j] = T[4 * i + j]; t[i] = T[4 * i + 3]; }
    ev.res(lvl, R, t, aff[0], aff[1], cutoff, rs);
    ev.hess(lvl, R, t, aff[0], aff[1], cutoff);
    std::memcpy(H, ev.Hm, sizeof(ev.Hm));
    std::memcpy(b, ev.bv, sizeof(ev.bv));
    if (rows) {
        const Level& L = h->g.l[lvl];
        const Warp w = make_warp(L, lvl, h->s, h->ph, R, t, aff[0], aff[1], cutoff);
        for (int i = 0; i < h->pc_n[lvl]; ++i) rows[i] = point_term(w, h->nw.data() + L.off, h->pc[L.off + i], i);
    }
}

// which as EDS_CT_*: 0 ref image, 1 new image (h x w x 3), 2 idepth, 3 weight sums (h x w), 4 the pc list (n x 4); returns the count
int ct_get_level(const HostCt* h, int which, int lvl, float* out) {
    const Level& L = h->g.l[lvl];
    const int px = L.w * L.h;
    if (which <= 1) {
        const Px* p = (which == 0 ? h->ref.data() : h->nw.data()) + L.off;
        for (int i = 0; i < px; ++i) { out[3 * i] = p[i].c; out[3 * i + 1] = p[i].dx; out[3 * i + 2] = p[i].dy; }
        return px;
    }
    if (which <= 3) {
        std::memcpy(out, (which == 2 ? h->idepth.data() : h->wsum.data()) + L.off, (size_t)px * sizeof(float));
        return px;
    }
    if (h->pc_n[lvl]) std::memcpy(out, h->pc.data() + L.off, (size_t)h->pc_n[lvl] * sizeof(Pc));
    return h->pc_n[lvl];
}

}  // extern "C"

#ifdef CT_STANDALONE
namespace {

struct Reader {
    FILE* f;
    template <class T> void get(T* p, size_t n) {
        if (n && std::fread(p, sizeof(T), n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); }
    }
    int i32() { int32_t v; get(&v, 1); return v; }
    float f32() { float v; get(&v, 1); return v; }
    double f64() { double v; get(&v, 1); return v; }
};

long n_tracks, n_ok, n_iters, n_entries;

void run_all(HostCt* h, const std::vector<double>& T, const std::vector<double>& aff, int coarsest, const double* min_res) {
    const int count = (int)aff.size() / 2;
    std::vector<TrackOut> out((size_t)count);
    ct_track(h, count, T.data(), aff.data(), coarsest, min_res, out.data());
    for (const TrackOut& o : out) {
        ++n_tracks; n_ok += o.ok;
        for (int l = 0; l < MAX_LEVELS; ++l) n_iters += o.iters[l];
    }
    std::vector<Term> rows((size_t)h->g.W * h->g.H);
    for (int l = 0; l < h->g.levels; ++l) {
        double rs[6], H[64], b[8];
        ct_calc_res(h, l, T.data(), aff.data(), h->s.coarse_cutoff_th, rs, H, b, rows.data());
        n_entries += h->pc_n[l];
    }
}

// inputs no caller should pass: the C API refuses most of them, the header must survive all of them
void hostile(int H, int W, int levels, const std::vector<float>& ref, const std::vector<float>& nw, const std::vector<float>& cp,
             const std::vector<float>& hdif) {
    const float nan = nan_f(), inf = 1.0f / 0.0f;
    const double dn = nan_d(), di = 1.0 / 0.0;
    const double min_res[5] = {dn, dn, dn, dn, dn};
    const double Ts[][12] = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, {dn, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, {1, 0, 0, di, 0, 1, 0, 0, 0, 0, 1, 0},
                             {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, dn}, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, {1e300, 0, 0, 0, 0, -1e300, 0, 0, 0, 0, 1, -1},
                             {1, 0, 0, 1e30, 0, 1, 0, -1e30, 0, 0, 1, 5}, {-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0}};
    const double affs[][2] = {{0, 0}, {dn, 0}, {0, di}, {800, 0}, {-800, 1e300}};
    const float calibs[][4] = {{40, 50, 30, 20}, {nan, 50, 30, 20}, {40, inf, 30, 20}, {0, 0, 0, 0}, {40, 50, nan, -inf}, {-40, -50, 1e30f, -1e30f}};
    const float exps[] = {1.0f, 0.0f, nan, inf, -1.0f};
    HostCt* h = ct_create(H, W, levels);
    const int n = (int)hdif.size();
    // hostile contributions: zero and negative HdiF, non-finite and far coordinates and idepths
    std::vector<float> cpb = cp, hdb = hdif;
    const float bad_xy[] = {nan, inf, -inf, 2147483648.0f, -2147483648.0f, 4294967296.0f, -0.75f, -1.5f, (float)W - 0.5f, (float)W - 0.51f, 1e30f};
    for (int i = 0; i < n; ++i) {
        if (i % 3 == 0) cpb[3 * i + (i / 3) % 2] = bad_xy[(i / 6) % 11];
        if (i % 5 == 0) cpb[3 * i + 2] = (i % 10) ? nan : -1.0f;
        if (i % 7 == 0) hdb[i] = (i % 14) ? 0.0f : -3.0f;
        if (i % 11 == 0) hdb[i] = (i % 22) ? nan : inf;
    }
    std::vector<float> img_bad = nw;
    for (size_t i = 0; i < img_bad.size(); i += 17) img_bad[i] = (i % 34) ? nan : inf;
    for (const auto& K : calibs)
        for (float e : exps) {
            ct_set_calib(h, K[0], K[1], K[2], K[3]);
            ct_set_ref(h, ref.data(), e, 0.0, 0.0, n, cpb.data(), hdb.data(), nullptr);
            ct_set_new(h, img_bad.data(), exps[0]);
            for (const auto& T : Ts)
                for (const auto& a : affs) run_all(h, std::vector<double>(T, T + 12), std::vector<double>(a, a + 2), levels - 1, min_res);
        }
    // the empty reference, and one with the well-formed contributions and non-finite affine state
    ct_set_calib(h, calibs[0][0], calibs[0][1], calibs[0][2], calibs[0][3]);
    ct_set_ref(h, ref.data(), 1.0f, 0.0, 0.0, 0, nullptr, nullptr, nullptr);
    ct_set_new(h, nw.data(), 1.0f);
    for (const auto& T : Ts) run_all(h, std::vector<double>(T, T + 12), std::vector<double>(affs[0], affs[0] + 2), levels - 1, min_res);
    ct_set_ref(h, img_bad.data(), 1.0f, dn, di, n, cp.data(), hdif.data(), nullptr);
    for (int m = 0; m < 4; ++m) {
        Params p = params_default();
        p.affine_opt_mode_a = (m & 1) ? -1.0f : 0.0f; p.affine_opt_mode_b = (m & 2) ? -1.0f : 0.0f;
        ct_set_params(h, &p);
        for (const auto& T : Ts) run_all(h, std::vector<double>(T, T + 12), std::vector<double>(affs[0], affs[0] + 2), 0, min_res);
    }
    ct_destroy(h);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    Reader r{std::fopen(argv[1], "rb")};
    if (!r.f) { std::perror(argv[1]); return 2; }
    const int ncases = r.i32();
    for (int c = 0; c < ncases; ++c) {
        const int H = r.i32(), W = r.i32(), levels = r.i32();
        Params s;
        r.get(&s, 1);
        float K[4];
        r.get(K, 4);
        HostCt* h = ct_create(H, W, levels);
        if (!h || !params_valid(s)) { std::fprintf(stderr, "case %d: bad shape or parameters\n", c); return 2; }
        ct_set_params(h, &s);
        ct_set_calib(h, K[0], K[1], K[2], K[3]);
        std::vector<float> ref((size_t)H * W), nw((size_t)H * W);
        r.get(ref.data(), ref.size());
        const float e_ref = r.f32();
        const double a = r.f64(), b = r.f64();
        const int n = r.i32();
        std::vector<float> cp((size_t)n * 3), hdif((size_t)n);
        r.get(cp.data(), cp.size()); r.get(hdif.data(), hdif.size());
        r.get(nw.data(), nw.size());
        const float e_new = r.f32();
        const int count = r.i32(), coarsest = r.i32();
        std::vector<double> T((size_t)count * 12), aff((size_t)count * 2);
        double min_res[5];
        r.get(T.data(), T.size()); r.get(aff.data(), aff.size()); r.get(min_res, 5);
        ct_set_ref(h, ref.data(), e_ref, a, b, n, cp.data(), hdif.data(), nullptr);
        ct_set_new(h, nw.data(), e_new);
        run_all(h, T, aff, coarsest, min_res);
        ct_destroy(h);
        if (c == 0) hostile(H, W, levels, ref, nw, cp, hdif);
    }
    std::fclose(r.f);
    std::printf("coarse standalone: %d cases; %ld tracks, %ld ok, %ld iterations, %ld list entries evaluated\n", ncases, n_tracks, n_ok, n_iters,
                n_entries);
    return 0;
}
#endif
