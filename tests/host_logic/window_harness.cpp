// csrc/eds_window.hpp on the CPU: a host object with the entry points of include/eds_hip_window.h that tests/window_harness.py binds,
// and — with -DWIN_STANDALONE — a program of its own that runs a dumped set of cases plus hostile inputs (for a sanitizer build; it is
// never loaded into python that way).  Built with g++ -ffp-contract=off.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../slam-eds_amd/csrc/eds_window.hpp"

using namespace edswin;

static_assert(sizeof(Precalc) == 27 * sizeof(float), "the python side writes a record as 27 floats");
static_assert(sizeof(PointOut) == 40 && sizeof(Params) == 32, "the python side reads these by words");

struct ResidualOut { int32_t* state; float* energy; int32_t* new_state; float *new_energy, *new_energy_wo, *ret; int32_t* active; float *cp, *proj, *J, *efJ, *JpJdF; };
struct PointsOut { float *Hdd, *bd, *Hcd, *HdiF, *bdSum, *idh; int32_t* nres; };

struct HostWin {
    int H, W, max_frames, n = 0, m = 0;
    Params s;
    Calib K;
    std::vector<Px> frames;
    std::vector<Point> pts;
    std::vector<float> ids, idz;
    std::vector<int32_t> res_first, res_point, res_target, state, new_state, active;
    std::vector<float> energy, new_energy, new_energy_wo, ret, cp, proj, J, efJ, JpJdF;
    std::vector<PointOut> pout;
    Tables tables() {
        Tables t = {m, res_point.data(), res_target.data(), state.data(), new_state.data(), active.data(), energy.data(), new_energy.data(),
                    new_energy_wo.data(), ret.data(), cp.data(), proj.data(), J.data(), efJ.data(), JpJdF.data()};
        return t;
    }
};

extern "C" {

int win_sizes(int* j_words, int* lanes) { *j_words = J_WORDS; *lanes = LANES; return (int)sizeof(Point); }

HostWin* win_create(int H, int W, int max_frames) {
    if (!shape_valid(H, W) || max_frames < 2 || max_frames > MAX_FRAMES) return nullptr;
    HostWin* h = new HostWin;
    h->H = H; h->W = W; h->max_frames = max_frames;
    h->s = params_default();
    h->K = make_calib(H, W, 1.0f, 1.0f, 0.0f, 0.0f);
    const Px zero = {0.0f, 0.0f, 0.0f, 0.0f};
    h->frames.assign((size_t)max_frames * H * W, zero);
    h->res_first.assign(1, 0);
    return h;
}
void win_destroy(HostWin* h) { delete h; }
int win_set_params(HostWin* h, const Params* p) { if (!params_valid(*p)) return -1; h->s = *p; return 0; }
void win_set_calib(HostWin* h, float fx, float fy, float cx, float cy) { h->K = make_calib(h->H, h->W, fx, fy, cx, cy); }
void win_set_frames(HostWin* h, int first, int count, const float* images) {
    const size_t px = (size_t)h->H * h->W;
    for (int f = 0; f < count; ++f) make_frame(h->H, h->W, images + f * px, h->W, h->frames.data() + (first + f) * px);
}
void win_get_frame(const HostWin* h, int f, float* out) {
    const size_t px = (size_t)h->H * h->W;
    const Px* p = h->frames.data() + f * px;
    for (size_t i = 0; i < px; ++i) { out[3 * i] = p[i].c; out[3 * i + 1] = p[i].dx; out[3 * i + 2] = p[i].dy; }
}

int win_set_points(HostWin* h, int n, const int32_t* host, const float* uv, const float* color, const float* weights, const float* ids, const float* idz) {
    uint32_t closed = 0;
    for (int i = 0; i < n; ++i) {
        if (host[i] < 0 || host[i] >= h->max_frames) return -1;
        if (i > 0 && host[i] != host[i - 1]) closed |= 1u << host[i - 1];
        if (closed >> host[i] & 1u) return -1;
    }
    h->pts.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        Point& p = h->pts[i];
        p.host = host[i]; p.u = uv[2 * i]; p.v = uv[2 * i + 1];
        for (int k = 0; k < 8; ++k) { p.color[k] = color[8 * i + k]; p.weights[k] = weights[8 * i + k]; }
    }
    h->ids.assign(ids, ids + n); h->idz.assign(idz, idz + n);
    h->n = n; h->m = 0;
    PointOut z;
    std::memset(&z, 0, sizeof(z));
    h->pout.assign((size_t)n, z);
    h->res_first.assign((size_t)n + 1, 0);
    return 0;
}
void win_set_idepths(HostWin* h, const float* ids, const float* idz) {
    for (int i = 0; i < h->n; ++i) { if (ids) h->ids[i] = ids[i]; if (idz) h->idz[i] = idz[i]; }
}

int win_set_residuals(HostWin* h, int m, const int32_t* point, const int32_t* target, const int32_t* state, const float* energy) {
    for (int i = 0; i < m; ++i) {
        if (point[i] < 0 || point[i] >= h->n || (i > 0 && point[i] < point[i - 1])) return -1;
        if (target[i] < 0 || target[i] >= h->max_frames || target[i] == h->pts[point[i]].host) return -1;
        if (state && (state[i] < 0 || state[i] > 2)) return -1;
    }
    h->m = m;
    const size_t mm = (size_t)m;
    h->res_point.assign(point, point + m); h->res_target.assign(target, target + m);
    h->state.assign(mm, ST_IN); if (state) h->state.assign(state, state + m);
    h->energy.assign(mm, 0.0f); if (energy) h->energy.assign(energy, energy + m);
    h->new_state.assign(mm, ST_OUTLIER); h->new_energy = h->energy; h->active.assign(mm, 0);
    h->new_energy_wo.assign(mm, 0.0f); h->ret.assign(mm, 0.0f); h->cp.assign(3 * mm, 0.0f); h->proj.assign(16 * mm, 0.0f);
    h->J.assign(J_WORDS * mm, 0.0f); h->efJ.assign(J_WORDS * mm, 0.0f); h->JpJdF.assign(8 * mm, 0.0f);
    h->res_first.assign((size_t)h->n + 1, 0);
    for (int i = 0; i < m; ++i) ++h->res_first[point[i] + 1];
    for (int p = 0; p < h->n; ++p) h->res_first[p + 1] += h->res_first[p];
    return 0;
}

int win_linearize(HostWin* h, int F, const float* precalc, const float* th, double* energy, int32_t* counts) {
    if (F < 2 || F > h->max_frames) return -1;
    for (int i = 0; i < F * F * 27; ++i) if (!finite_f(precalc[i])) return -1;
    for (int i = 0; i < F; ++i) if (!finite_f(th[i])) return -1;
    for (int i = 0; i < h->n; ++i) if (h->pts[i].host >= F) return -1;
    for (int i = 0; i < h->m; ++i) if (h->res_target[i] >= F) return -1;
    int32_t c[3] = {0, 0, 0};
    double e = 0.0;
    if (h->m) e = linearize_serial(h->K, h->s, F, reinterpret_cast<const Precalc*>(precalc), th, h->frames.data(), h->pts.data(), h->ids.data(), h->idz.data(), h->tables(), c);
    if (energy) *energy = e;
    if (counts) for (int k = 0; k < 3; ++k) counts[k] = c[k];
    return 0;
}
// the three per-residual / per-point stages over the points p0 .. p1 - 1 only (their residuals are one run of the table): slices of
// different points touch different entries, so a pool of threads may run them side by side; the energy is folded afterwards, in the
// header's order, from the returns every slice left in the table
void win_linearize_points(HostWin* h, int F, const float* precalc, const float* th, int p0, int p1) {
    const Tables t = h->tables();
    for (int i = h->res_first[p0]; i < h->res_first[p1]; ++i)
        t.ret[i] = linearize_one(h->K, h->s, F, reinterpret_cast<const Precalc*>(precalc), th, h->frames.data(), h->pts.data(), h->ids.data(), h->idz.data(), t, i);
}
double win_linearize_fold(HostWin* h, int32_t* counts) {
    double part[LANES];
    for (int l = 0; l < LANES; ++l) part[l] = 0.0;
    counts[0] = counts[1] = counts[2] = 0;
    for (int i = 0; i < h->m; ++i) { part[i % LANES] += (double)h->ret[i]; ++counts[h->new_state[i]]; }
    return edsct::reduce_lanes(part);
}
void win_apply_points(HostWin* h, int copy_jacobians, int p0, int p1) {
    const Tables t = h->tables();
    const ResState r = {t.state, t.energy, t.active, t.new_state, t.new_energy, t.J, t.efJ, t.JpJdF};
    for (int i = h->res_first[p0]; i < h->res_first[p1]; ++i) apply_one(r, i, copy_jacobians != 0);
}
int win_point_hessians_points(HostWin* h, const float* prior, const float* delta, const float* lf, int shift, int p0, int p1) {
    const float zero[6] = {0, 0, 0, 0, 0, 0};
    const Tables t = h->tables();
    int nres = 0;
    for (int p = p0; p < p1; ++p) {
        h->pout[p] = point_sums(t.active, t.efJ, h->res_first[p], h->res_first[p + 1], prior ? prior[p] : 0.0f, delta ? delta[p] : 0.0f, lf ? lf + 6 * p : zero, shift != 0);
        nres += h->pout[p].nres;
    }
    return nres;
}

void win_apply(HostWin* h, int copy_jacobians) { if (h->m) apply_serial(h->tables(), copy_jacobians != 0); }
int win_point_hessians(HostWin* h, const float* prior, const float* delta, const float* lf, int shift) {
    return h->n ? points_serial(h->n, h->res_first.data(), h->tables(), prior, delta, lf, shift != 0, h->pout.data()) : 0;
}

// eds_win_accumulate: returns nres, or -1 for what the entry point refuses
int win_acc_size(int F) { return acc_size(F); }
int win_accumulate(HostWin* h, int F, const double* adH, const double* adT, const float* prior, const float* delta, const float* lf, int shift,
                   double* HA, double* bA, double* Hsc, double* bsc, double* acc_out) {
    if (F < 2 || F > h->max_frames) return -1;
    for (int i = 0; i < F * F * 64; ++i) if (!std::isfinite(adH[i]) || !std::isfinite(adT[i])) return -1;
    for (int p = 0; p < h->n; ++p) if (h->pts[p].host >= F) return -1;
    std::vector<int32_t> res_of((size_t)h->n * F, -1), first(9, 0);
    for (int i = 0; i < h->m; ++i) {
        if (h->res_target[i] >= F) return -1;
        int32_t& slot = res_of[(size_t)h->res_point[i] * F + h->res_target[i]];
        if (slot >= 0) return -1;
        slot = i;
    }
    for (int p = 1; p < h->n; ++p) if (h->pts[p].host < h->pts[p - 1].host) return -1;
    for (int f = 0, p = 0; f < 9; ++f) { first[f] = p; while (p < h->n && h->pts[p].host == f) ++p; }
    const int nres = win_point_hessians(h, prior, delta, lf, shift);
    const Tables t = h->tables();
    const AccIn in = {F, lf ? 1 : 0, first.data(), res_of.data(), t.active, t.efJ, t.JpJdF, h->pout.data(), lf};
    std::vector<double> acc((size_t)acc_size(F), 0.0);
    accumulate_serial(in, acc.data());
    const size_t N = 4 + 8 * (size_t)F;
    std::vector<double> a(N * N), b(N), c(N * N), d(N);
    stitch_serial(F, acc.data(), adH, adT, a.data(), b.data(), c.data(), d.data());
    if (HA) std::memcpy(HA, a.data(), a.size() * 8);
    if (bA) std::memcpy(bA, b.data(), b.size() * 8);
    if (Hsc) std::memcpy(Hsc, c.data(), c.size() * 8);
    if (bsc) std::memcpy(bsc, d.data(), d.size() * 8);
    if (acc_out) std::memcpy(acc_out, acc.data(), acc.size() * 8);
    return nres;
}

// both stitches entry by entry (what the device's stitch kernel runs): out = H_A, b_A, H_sc, b_sc one after the other
void win_stitch_entries(int F, const double* acc, const double* adH, const double* adT, double* out) {
    for (int e = 0; e < stitch_words(F); ++e) stitch_entry(F, acc, adH, adT, e, out);
}

void win_get_residuals(const HostWin* h, const ResidualOut* o) {
    const size_t m = (size_t)h->m;
    if (!m) return;
#define WIN_COPY(dst, src, k) if (o->dst) std::memcpy(o->dst, h->src.data(), (k) * m * 4)
    WIN_COPY(state, state, 1); WIN_COPY(energy, energy, 1); WIN_COPY(new_state, new_state, 1); WIN_COPY(new_energy, new_energy, 1);
    WIN_COPY(new_energy_wo, new_energy_wo, 1); WIN_COPY(ret, ret, 1); WIN_COPY(active, active, 1); WIN_COPY(cp, cp, 3); WIN_COPY(proj, proj, 16);
    WIN_COPY(J, J, J_WORDS); WIN_COPY(efJ, efJ, J_WORDS); WIN_COPY(JpJdF, JpJdF, 8);
#undef WIN_COPY
}
void win_get_points(const HostWin* h, const PointsOut* o) {
    for (int i = 0; i < h->n; ++i) {
        const PointOut& p = h->pout[i];
        if (o->Hdd) o->Hdd[i] = p.Hdd_accAF;
        if (o->bd) o->bd[i] = p.bd_accAF;
        if (o->Hcd) std::memcpy(o->Hcd + 4 * i, p.Hcd_accAF, 16);
        if (o->HdiF) o->HdiF[i] = p.HdiF;
        if (o->bdSum) o->bdSum[i] = p.bdSumF;
        if (o->idh) o->idh[i] = p.idepth_hessian;
        if (o->nres) o->nres[i] = p.nres;
    }
}

}  // extern "C"

#ifdef WIN_STANDALONE
namespace {

struct Reader {
    FILE* f;
    template <class T> void get(T* p, size_t n) {
        if (n && std::fread(p, sizeof(T), n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); }
    }
    int i32() { int32_t v; get(&v, 1); return v; }
    template <class T> std::vector<T> vec(size_t n) { std::vector<T> v(n); get(v.data(), n); return v; }
};

struct Case {
    int H, W, F, n, m;
    Params s;
    float K[4];
    std::vector<float> images, uv, color, weights, ids, idz, ids2, precalc, th, energy, prior, delta, lf;
    std::vector<int32_t> host, point, target, state;
    std::vector<double> adH, adT;
    int shift;
};

Case read_case(Reader& r) {
    Case c;
    c.H = r.i32(); c.W = r.i32(); c.F = r.i32(); c.n = r.i32(); c.m = r.i32(); c.shift = r.i32();
    r.get(&c.s, 1); r.get(c.K, 4);
    const size_t n = (size_t)c.n, m = (size_t)c.m;
    c.images = r.vec<float>((size_t)c.F * c.H * c.W);
    c.host = r.vec<int32_t>(n); c.uv = r.vec<float>(2 * n); c.color = r.vec<float>(8 * n); c.weights = r.vec<float>(8 * n);
    c.ids = r.vec<float>(n); c.idz = r.vec<float>(n); c.ids2 = r.vec<float>(n);
    c.point = r.vec<int32_t>(m); c.target = r.vec<int32_t>(m); c.state = r.vec<int32_t>(m); c.energy = r.vec<float>(m);
    c.precalc = r.vec<float>((size_t)c.F * c.F * 27); c.th = r.vec<float>((size_t)c.F);
    c.prior = r.vec<float>(n); c.delta = r.vec<float>(n); c.lf = r.vec<float>(6 * n);
    c.adH = r.vec<double>((size_t)c.F * c.F * 64); c.adT = r.vec<double>((size_t)c.F * c.F * 64);
    return c;
}

long long g_res = 0, g_counts[3] = {0, 0, 0}, g_nres = 0, g_refused = 0, g_acc = 0, g_acc_refused = 0, g_nonfinite = 0;

// win_accumulate with the given adjoints; what it returns goes into a checksum so that nothing is optimised away
void accumulate_once(HostWin* h, const Case& c, const double* adH, const double* adT) {
    const size_t N = 4 + 8 * (size_t)c.F;
    std::vector<double> HA(N * N), bA(N), Hs(N * N), bs(N), acc((size_t)win_acc_size(c.F));
    const int nres = win_accumulate(h, c.F, adH, adT, c.prior.data(), c.delta.data(), c.lf.data(), c.shift, HA.data(), bA.data(), Hs.data(), bs.data(), acc.data());
    if (nres < 0) { ++g_acc_refused; return; }
    ++g_acc;
    const long long before = g_nonfinite;
    for (double v : HA) if (!std::isfinite(v)) ++g_nonfinite;
    for (double v : Hs) if (!std::isfinite(v)) ++g_nonfinite;
    // the entry-wise stitch (the device kernel's code) gives the block-wise one's bits wherever everything is finite
    std::vector<double> e((size_t)stitch_words(c.F));
    win_stitch_entries(c.F, acc.data(), adH, adT, e.data());
    if (g_nonfinite == before &&
        (std::memcmp(e.data(), HA.data(), N * N * 8) || std::memcmp(e.data() + N * N, bA.data(), N * 8) || std::memcmp(e.data() + N * N + N, Hs.data(), N * N * 8) ||
         std::memcmp(e.data() + 2 * N * N + N, bs.data(), N * 8))) { std::fprintf(stderr, "entry-wise stitch differs\n"); std::exit(11); }
}

HostWin* open_case(const Case& c) {
    HostWin* h = win_create(c.H, c.W, c.F);
    if (!h) { std::fprintf(stderr, "shape refused\n"); std::exit(3); }
    win_set_params(h, &c.s);
    win_set_calib(h, c.K[0], c.K[1], c.K[2], c.K[3]);
    win_set_frames(h, 0, c.F, c.images.data());
    if (win_set_points(h, c.n, c.host.data(), c.uv.data(), c.color.data(), c.weights.data(), c.ids.data(), c.idz.data())) std::exit(4);
    if (win_set_residuals(h, c.m, c.point.data(), c.target.data(), c.state.data(), c.energy.data())) std::exit(5);
    return h;
}

void round_trip(HostWin* h, const Case& c, const float* precalc, const float* th) {
    double e;
    int32_t cnt[3];
    if (win_linearize(h, c.F, precalc, th, &e, cnt)) { ++g_refused; return; }
    win_apply(h, 1);
    g_nres += win_point_hessians(h, c.prior.data(), c.delta.data(), c.lf.data(), c.shift);
    accumulate_once(h, c, c.adH.data(), c.adT.data());
    g_res += h->m;
    for (int k = 0; k < 3; ++k) g_counts[k] += cnt[k];
}

void hostile(const Case& c) {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float bad[] = {nan, inf, -inf, 0.0f, -1.0f, 1e30f, -1e30f, 1e-30f};
    for (float v : bad) {
        // refused: a non-finite precalc or threshold; accepted: zero and huge ones
        HostWin* h = open_case(c);
        std::vector<float> pc(c.precalc.size(), v), th(c.th.size(), v);
        round_trip(h, c, pc.data(), c.th.data());
        round_trip(h, c, c.precalc.data(), th.data());
        for (size_t k = 0; k < pc.size(); k += 5) { pc = c.precalc; pc[k] = v; round_trip(h, c, pc.data(), c.th.data()); }
        // idepths NaN, negative, 1e30
        std::vector<float> id((size_t)c.n, v);
        win_set_idepths(h, id.data(), id.data());
        round_trip(h, c, c.precalc.data(), c.th.data());
        win_destroy(h);
    }
    {   // a point on every border pixel, towards every other frame, with its idepth as it is and as 0
        HostWin* h = open_case(c);
        std::vector<int32_t> host, point, target;
        std::vector<float> uv;
        for (int y = 0; y < c.H; ++y)
            for (int x = 0; x < c.W; ++x)
                if (x < 4 || y < 4 || x >= c.W - 4 || y >= c.H - 4) { host.push_back(0); uv.push_back((float)x); uv.push_back((float)y); }
        const int n = (int)host.size();
        std::vector<float> col(8 * (size_t)n, 100.0f), wgt(8 * (size_t)n, 1.0f), id((size_t)n, 0.0f);
        for (int p = 0; p < n; ++p)
            for (int t = 1; t < c.F; ++t) { point.push_back(p); target.push_back(t); }
        Case b = c;
        b.prior.assign((size_t)n, 0.0f); b.delta.assign((size_t)n, 0.0f); b.lf.assign(6 * (size_t)n, 0.0f);
        if (win_set_points(h, n, host.data(), uv.data(), col.data(), wgt.data(), id.data(), id.data())) std::exit(6);
        if (win_set_residuals(h, (int)point.size(), point.data(), target.data(), nullptr, nullptr)) std::exit(7);
        round_trip(h, b, c.precalc.data(), c.th.data());
        // the identity warp keeps border points on the border: the bounds test alone stands between them and the image's edge
        std::vector<float> ident((size_t)c.F * c.F * 27, 0.0f);
        for (int k = 0; k < c.F * c.F; ++k) { float* r = ident.data() + 27 * k; r[0] = r[4] = r[8] = r[12] = r[16] = r[20] = 1.0f; r[24] = 1.0f; }
        round_trip(h, b, ident.data(), c.th.data());
        // the empty window
        win_set_residuals(h, 0, nullptr, nullptr, nullptr, nullptr);
        round_trip(h, b, c.precalc.data(), c.th.data());
        win_set_points(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
        round_trip(h, b, c.precalc.data(), c.th.data());
        win_destroy(h);
    }
    {   // adjoints: NaN and inf (all, and in one word) are refused; zero, -1, 1e30 and 1e-30 run through both stitches
        HostWin* h = open_case(c);
        round_trip(h, c, c.precalc.data(), c.th.data());
        const double dnan = std::numeric_limits<double>::quiet_NaN(), dinf = std::numeric_limits<double>::infinity();
        const double badd[] = {dnan, dinf, -dinf, 0.0, -1.0, 1e30, -1e30, 1e-30, 1e300};
        for (double v : badd) {
            std::vector<double> a(c.adH.size(), v);
            accumulate_once(h, c, a.data(), c.adT.data());
            accumulate_once(h, c, c.adH.data(), a.data());
            accumulate_once(h, c, a.data(), a.data());
            a = c.adT; a[a.size() - 1] = v;
            accumulate_once(h, c, c.adH.data(), a.data());
        }
        // a point with two residuals towards one target is refused; F below a target is refused
        if (c.n >= 1 && c.F >= 3) {
            const int32_t pt[2] = {0, 0}, tg[2] = {c.host[0] == 1 ? 2 : 1, c.host[0] == 1 ? 2 : 1};
            if (win_set_residuals(h, 2, pt, tg, nullptr, nullptr)) std::exit(10);
            round_trip(h, c, c.precalc.data(), c.th.data());
            Case two = c; two.F = 2;
            accumulate_once(h, two, c.adH.data(), c.adT.data());
        }
        win_destroy(h);
    }
    {   // thresholds 0
        HostWin* h = open_case(c);
        std::vector<float> th(c.th.size(), 0.0f);
        round_trip(h, c, c.precalc.data(), th.data());
        Params p = c.s;
        p.huber_th = nan;
        if (win_set_params(h, &p) == 0) std::exit(8);
        p.huber_th = 0.0f;
        if (win_set_params(h, &p) == 0) std::exit(9);
        win_destroy(h);
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    Reader r = {std::fopen(argv[1], "rb")};
    if (!r.f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const int n_cases = r.i32();
    for (int k = 0; k < n_cases; ++k) {
        const Case c = read_case(r);
        HostWin* h = open_case(c);
        round_trip(h, c, c.precalc.data(), c.th.data());
        win_set_idepths(h, c.ids2.data(), nullptr);
        round_trip(h, c, c.precalc.data(), c.th.data());
        win_destroy(h);
        if (c.n <= 64) hostile(c);
    }
    std::fclose(r.f);
    std::printf("window standalone: %d cases; %lld residuals linearized, %lld IN, %lld OOB, %lld OUTLIER, %lld active added, %lld calls refused; "
                "%lld accumulates, %lld refused, %lld non-finite stitched entries\n",
                n_cases, g_res, g_counts[0], g_counts[1], g_counts[2], g_nres, g_refused, g_acc, g_acc_refused, g_nonfinite);
    return 0;
}
#endif
