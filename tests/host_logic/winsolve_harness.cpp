// csrc/eds_winsolve.hpp on the CPU: a host object with the entry points of include/eds_hip_winsolve.h over the HostWin of
// window_harness.cpp (included whole: its functions are this library's too), bound by tests/winsolve_harness.py, and — with
// -DWSV_STANDALONE — a program of its own that runs a dumped set of cases plus hostile inputs (for a sanitizer build; it is never
// loaded into python that way).  Built with g++ -ffp-contract=off.  The order of the steps is the device's (csrc/eds_winsolve.hip).
#include "window_harness.cpp"

#include "../../slam-eds_amd/csrc/eds_winsolve.hpp"

using namespace edswsv;

enum { RC_OK = 0, RC_INVALID = -1, RC_NOT_USABLE = -3, RC_STATE = -4 };

struct WsvOut { float* adHTdeltaF; int32_t* is_linearized; float *res_toZeroF, *resApprox, *lf; double *HFinal, *bFinal; float* xAd; double* frame_step;
                float *step, *idepth_scaled, *priorF; };
struct WsvStats { int32_t res_in_a, res_in_l, orth_x, orth_system; double lambda; };

struct HostWsv {
    HostWin* w = nullptr;
    int F = 0;
    bool valid = false, lf_on = false, have_backup = false, have_step = false, have_system = false;
    std::vector<int32_t> lin, first, res_of;
    std::vector<float> adF, adht, cF, prior, delta, lf, rtz, res_approx, xAd, step, backup;
    std::vector<double> ad, vec, work, stL, accL, acc, stitched, last_x;
    Lin lin_of() const {
        Lin t = {F, w->res_first.data(), w->res_point.data(), w->res_target.data(), w->active.data(), lin.data(), w->pts.data(), w->efJ.data(), rtz.data(),
                 res_approx.data(), adht.data(), cF.data(), delta.data(), prior.data()};
        return t;
    }
};

namespace {

bool fin(const double* x, size_t n) { for (size_t i = 0; i < n; ++i) if (!std::isfinite(x[i])) return false; return true; }
bool fin(const float* x, size_t n) { for (size_t i = 0; i < n; ++i) if (!std::isfinite(x[i])) return false; return true; }

// eds_win_accumulate's maps; false for what it refuses
bool build_maps(HostWsv* s) {
    HostWin* h = s->w;
    const int F = s->F;
    s->res_of.assign((size_t)h->n * F, -1);
    s->first.assign(9, 0);
    for (int p = 0; p < h->n; ++p) if (h->pts[p].host >= F) return false;
    for (int i = 0; i < h->m; ++i) {
        if (h->res_target[i] >= F) return false;
        int32_t& slot = s->res_of[(size_t)h->res_point[i] * F + h->res_target[i]];
        if (slot >= 0) return false;
        slot = i;
    }
    for (int p = 1; p < h->n; ++p) if (h->pts[p].host < h->pts[p - 1].host) return false;
    for (int f = 0, p = 0; f < 9; ++f) { s->first[f] = p; while (p < h->n && h->pts[p].host == f) ++p; }
    return true;
}
AccIn acc_in(HostWsv* s, int mode, const int32_t* sel) {
    HostWin* h = s->w;
    AccIn in = {s->F, 1, s->first.data(), s->res_of.data(), h->active.data(), h->efJ.data(), h->JpJdF.data(), h->pout.data(), s->lf.data(),
                mode, s->lin.data(), s->res_approx.data(), sel};
    return in;
}
void acc_words(const AccIn& in, int words, double* acc) {       // accumulate_serial over the first `words` words
    for (int j = 0; j < words; ++j) {
        const int hh = acc_host(in.F, j);
        double part[LANES];
        for (int l = 0; l < LANES; ++l) part[l] = 0.0;
        for (int p = in.first[hh]; p < in.first[hh + 1]; ++p) part[(p - in.first[hh]) % LANES] += acc_value(in, j, p);
        acc[j] = edsct::reduce_lanes(part);
    }
}
void res_approx_pass(HostWsv* s, int mode) {
    const Lin t = s->lin_of();
    for (int r = 0; r < s->w->m; ++r)
        if (s->lin[r]) for (int j = 0; j < 8; ++j) s->res_approx[(size_t)r * 8 + j] = res_approx_tap(t, mode, r, j);
}
int lf_pass(HostWsv* s, int mode, const int32_t* sel) {
    const Lin t = s->lin_of();
    int added = 0;
    for (int p = 0; p < s->w->n; ++p) if (!sel || sel[p]) added += lf_sums(t, mode, p, s->lf.data() + 6 * (size_t)p);
    return added;
}
int points_pass(HostWsv* s, int mode, const int32_t* sel, bool shift) {
    HostWin* h = s->w;
    int total = 0;
    for (int p = 0; p < h->n; ++p) {
        if (sel && !sel[p]) continue;
        int added = 0;
        h->pout[p] = point_sums_mode(h->active.data(), s->lin.data(), h->efJ.data(), h->res_first[p], h->res_first[p + 1], s->prior[p], s->delta[p],
                                     s->lf.data() + 6 * (size_t)p, shift, mode, &added);
        total += added;
    }
    return total;
}

}  // namespace

extern "C" {

HostWsv* wsv_create(HostWin* w) { HostWsv* s = new HostWsv; s->w = w; return s; }
void wsv_destroy(HostWsv* s) { delete s; }
void wsv_invalidate(HostWsv* s) { s->valid = false; s->lf_on = false; s->have_backup = s->have_step = s->have_system = false; }

int wsv_set_state(HostWsv* s, int F, const double* adHost, const double* adTarget, const double* delta, const double* prior, const double* delta_prior,
                  const double* cPrior, const double* cDelta, const float* priorF, const float* deltaF) {
    HostWin* h = s->w;
    if (F < 2 || F > h->max_frames) return RC_INVALID;
    if (!adHost || !adTarget || !delta || !prior || !delta_prior || !cPrior || !cDelta) return RC_INVALID;
    for (int p = 0; p < h->n; ++p) if (h->pts[p].host >= F) return RC_INVALID;
    for (int i = 0; i < h->m; ++i) if (h->res_target[i] >= F) return RC_INVALID;
    const size_t adw = (size_t)F * F * 64, n = (size_t)h->n, m = (size_t)h->m;
    if (!fin(adHost, adw) || !fin(adTarget, adw) || !fin(delta, 8 * (size_t)F) || !fin(prior, 8 * (size_t)F) || !fin(delta_prior, 8 * (size_t)F) ||
        !fin(cPrior, 4) || !fin(cDelta, 4) || (priorF && !fin(priorF, n)) || (deltaF && !fin(deltaF, n)))
        return RC_INVALID;
    s->adF.assign(2 * adw, 0.0f); s->adht.assign((size_t)F * F * 8, 0.0f); s->cF.assign(8, 0.0f);
    for (size_t i = 0; i < adw; ++i) { s->adF[i] = (float)adHost[i]; s->adF[adw + i] = (float)adTarget[i]; }
    for (int hh = 0; hh < F; ++hh)
        for (int t = 0; t < F; ++t) {
            const size_t idx = (size_t)hh + (size_t)F * t;
            adht_delta(s->adF.data() + 64 * idx, s->adF.data() + adw + 64 * idx, delta + 8 * hh, delta + 8 * t, s->adht.data() + 8 * idx);
        }
    s->ad.assign(adHost, adHost + adw); s->ad.insert(s->ad.end(), adTarget, adTarget + adw);
    s->vec.assign((size_t)4 * MAX_N, 0.0);
    for (int k = 0; k < 4; ++k) {
        s->cF[k] = (float)cDelta[k]; s->cF[4 + k] = (float)cPrior[k];
        s->vec[k] = (double)s->cF[k]; s->vec[MAX_N + k] = cPrior[k]; s->vec[2 * MAX_N + k] = cPrior[k] * (double)s->cF[k]; s->vec[3 * MAX_N + k] = (double)s->cF[k];
    }
    for (int i = 0; i < 8 * F; ++i) {
        s->vec[4 + i] = delta[i]; s->vec[MAX_N + 4 + i] = prior[i]; s->vec[2 * MAX_N + 4 + i] = prior[i] * delta_prior[i]; s->vec[3 * MAX_N + 4 + i] = delta_prior[i];
    }
    s->prior.assign(n, 0.0f); if (priorF) s->prior.assign(priorF, priorF + n);
    s->delta.assign(n, 0.0f); if (deltaF) s->delta.assign(deltaF, deltaF + n);
    s->lf.assign(6 * n, 0.0f); s->step.assign(n, 0.0f); s->backup.assign(n, 0.0f);
    s->lin.assign(m, 0); s->rtz.assign(8 * m, 0.0f); s->res_approx.assign(8 * m, 0.0f);
    s->xAd.assign(64 * 8 + 4, 0.0f);
    s->work.assign((size_t)work_words(), 0.0); s->stL.assign((size_t)MAX_N * (MAX_N + 1), 0.0);
    s->accL.assign((size_t)acc_size(8), 0.0); s->acc.assign((size_t)acc_size(8), 0.0); s->stitched.assign((size_t)stitch_words(8), 0.0);
    s->F = F; s->valid = true; s->lf_on = false; s->have_backup = s->have_step = s->have_system = false;
    return RC_OK;
}

int wsv_fix_linearization(HostWsv* s, const int32_t* select) {
    if (!s->valid) return RC_STATE;
    if (!select && s->w->m) return RC_INVALID;
    const Lin t = s->lin_of();
    for (int r = 0; r < s->w->m; ++r) {
        if (!select[r]) continue;
        for (int j = 0; j < 8; ++j) s->rtz[(size_t)r * 8 + j] = fix_tap(t, r, j);
        s->lin[r] = 1;
    }
    return RC_OK;
}

int wsv_solve(HostWsv* s, int iteration, double lambda, int mode, int have_first_frame, const double* HM, const double* bM, const double* projector,
              double* x, double* lastHS, double* lastbS, WsvStats* stats) {
    if (!s->valid) return RC_STATE;
    HostWin* h = s->w;
    const int F = s->F, N = 4 + 8 * F;
    const size_t NN = (size_t)N * N;
    if (!mode_valid(mode)) return RC_INVALID;
    if (iteration < 0 || !std::isfinite(lambda) || lambda < 0) return RC_INVALID;
    if (have_first_frame != 0 && have_first_frame != 1) return RC_INVALID;
    if (!HM || !bM || !x) return RC_INVALID;
    if (!fin(HM, NN) || !fin(bM, (size_t)N) || (projector && !fin(projector, NN))) return RC_INVALID;
    if (!build_maps(s)) return RC_INVALID;
    lambda = mode_lambda(mode, lambda);
    const int system = (mode & SOLVER_ORTHOGONALIZE_SYSTEM) ? 1 : 0;
    const int orth_system = system && !have_first_frame && projector ? 1 : 0;
    const int orth_x = mode_orth_x(mode, iteration) && projector ? 1 : 0;
    double* st = s->stitched.data();
    Sys sys = {N, system, orth_system, lambda, st, st + NN, st + NN + N, st + 2 * NN + N, s->stL.data(), s->stL.data() + NN, s->vec.data(), s->work.data()};
    std::memcpy(sys.mat(W_HM), HM, NN * 8);
    std::memcpy(sys.v(V_BM), bM, (size_t)N * 8);
    if (projector) std::memcpy(sys.mat(W_P), projector, NN * 8);
    res_approx_pass(s, 1);
    const int res_l = lf_pass(s, 1, nullptr);
    s->lf_on = true;
    acc_words(acc_in(s, 1, nullptr), F * F * TOP_WORDS, s->accL.data());
    for (int e = 0; e < N * (N + 1); ++e) stitch_entry(F, s->accL.data(), s->ad.data(), s->ad.data() + (size_t)F * F * 64, e, s->stL.data());
    const int res_a = points_pass(s, 0, nullptr, true);
    acc_words(acc_in(s, 0, nullptr), acc_size(F), s->acc.data());
    for (int e = 0; e < stitch_words(F); ++e) stitch_entry(F, s->acc.data(), s->ad.data(), s->ad.data() + (size_t)F * F * 64, e, st);
    for (int e = 0; e < N * (N + 1); ++e) assemble(sys, 0, e);
    if (system) {
        if (orth_system) {
            for (int e = 0; e < N * (N + 1); ++e) assemble(sys, 1, e);
            for (int e = 0; e < N * (N + 1); ++e) assemble(sys, 2, e);
        }
        for (int e = 0; e < N * (N + 1); ++e) assemble(sys, 3, e);
    }
    int32_t flag[4] = {0, 0, 0, 0};
    const SolveIo io = {N, F, orth_x, sys.mat(W_HF), sys.v(V_BF), sys.mat(W_P), s->adF.data(), sys.v(V_X), s->xAd.data(), flag, nullptr, nullptr};
    SolveMem* mem = new SolveMem;
    solve_serial(io, *mem);
    delete mem;
    if (!flag[0]) {
        const Lin t = s->lin_of();
        for (int p = 0; p < h->n; ++p) s->step[p] = point_step(t, h->pout[p], s->lf.data() + 6 * (size_t)p, h->JpJdF.data(), s->xAd.data(), p);
    }
    std::memcpy(x, sys.v(V_X), (size_t)N * 8);
    if (lastHS) std::memcpy(lastHS, sys.mat(W_LASTH), NN * 8);
    if (lastbS) std::memcpy(lastbS, sys.v(V_LASTB), (size_t)N * 8);
    if (stats) { stats->res_in_a = res_a; stats->res_in_l = res_l; stats->orth_x = orth_x; stats->orth_system = orth_system; stats->lambda = lambda; }
    s->have_system = true;
    s->last_x.assign(x, x + N);
    if (flag[0]) return RC_NOT_USABLE;
    s->have_step = true;
    return RC_OK;
}

int wsv_backup_idepths(HostWsv* s) {
    if (!s->valid) return RC_STATE;
    for (int p = 0; p < s->w->n; ++p) s->backup[p] = idepth_of(s->w->ids[p], s->w->s.scale_idepth);
    s->have_backup = true;
    return RC_OK;
}
int wsv_step_idepths(HostWsv* s, float fac) {
    if (!s->valid) return RC_STATE;
    if (!std::isfinite(fac)) return RC_INVALID;
    if (!s->have_backup || !s->have_step) return RC_STATE;
    for (int p = 0; p < s->w->n; ++p) s->w->ids[p] = stepped_idepth_scaled(s->backup[p], fac, s->step[p], s->w->s.scale_idepth);
    return RC_OK;
}

int wsv_l_energy(HostWsv* s, double* energy) {
    if (!s->valid) return RC_STATE;
    if (!build_maps(s)) return RC_INVALID;
    const Lin t = s->lin_of();
    double total = 0.0;
    for (int hh = 0; hh < s->F; ++hh) {
        double part[LANES];
        for (int l = 0; l < LANES; ++l) part[l] = 0.0;
        for (int p = s->first[hh]; p < s->first[hh + 1]; ++p) part[(p - s->first[hh]) % LANES] += lenergy_point(t, p);
        total += edsct::reduce_lanes(part);
    }
    *energy = lenergy_priors(s->F, s->vec.data(), s->cF.data()) + total;
    return RC_OK;
}
// the per-point values and the terms of their sums, for the oracle's bound
void wsv_l_energy_points(HostWsv* s, double* out) {
    const Lin t = s->lin_of();
    for (int p = 0; p < s->w->n; ++p) out[p] = lenergy_point(t, p);
}

int wsv_m_energy(HostWsv* s, const double* HM, const double* bM, double* energy) {
    if (!s->valid) return RC_STATE;
    const int N = 4 + 8 * s->F;
    if (!HM || !bM || !energy) return RC_INVALID;
    if (!fin(HM, (size_t)N * N) || !fin(bM, (size_t)N)) return RC_INVALID;
    double e = 0.0;
    for (int i = 0; i < N; ++i) e += s->vec[i] * menergy_row(N, HM, bM, s->vec.data(), i);
    *energy = e;
    return RC_OK;
}

int wsv_marginalize_points(HostWsv* s, const int32_t* marg, float prior_fac, double weight_fac, double* HM, double* bM, int32_t* res_in_m) {
    if (!s->valid) return RC_STATE;
    HostWin* h = s->w;
    if (!HM || !bM || (!marg && h->n)) return RC_INVALID;
    const int F = s->F, N = 4 + 8 * F;
    const size_t NN = (size_t)N * N;
    if (!std::isfinite(prior_fac) || !std::isfinite(weight_fac) || !fin(HM, NN) || !fin(bM, (size_t)N)) return RC_INVALID;
    if (!build_maps(s)) return RC_INVALID;
    for (int r = 0; r < h->m; ++r) if (marg[h->res_point[r]] && h->active[r] && !s->lin[r]) return RC_STATE;
    for (int p = 0; p < h->n; ++p) if (marg[p]) s->prior[p] *= prior_fac;
    res_approx_pass(s, 2);
    const int added = lf_pass(s, 2, marg);
    s->lf_on = true;
    points_pass(s, 2, marg, false);
    acc_words(acc_in(s, 2, marg), acc_size(F), s->acc.data());
    double* st = s->stitched.data();
    for (int e = 0; e < stitch_words(F); ++e) stitch_entry(F, s->acc.data(), s->ad.data(), s->ad.data() + (size_t)F * F * 64, e, st);
    const int half = N * (N + 1);
    for (int e = 0; e < half; ++e) {
        double* io = e < (int)NN ? HM + e : bM + (e - NN);
        *io = *io + weight_fac * (st[e] - st[half + e]);
    }
    if (res_in_m) *res_in_m = added;
    return RC_OK;
}

int wsv_get(HostWsv* s, const WsvOut* o) {
    if (!s->valid) return RC_STATE;
    const int F = s->F, N = 4 + 8 * F;
    const size_t NN = (size_t)N * N, n = (size_t)s->w->n, m = (size_t)s->w->m;
    if ((o->HFinal || o->bFinal || o->xAd || o->frame_step) && !s->have_system) return RC_STATE;
#define WSV_COPY(dst, src, count) if (o->dst && (count) != 0) std::memcpy(o->dst, src, (count) * sizeof(*o->dst))
    WSV_COPY(adHTdeltaF, s->adht.data(), (size_t)F * F * 8);
    WSV_COPY(is_linearized, s->lin.data(), m);
    WSV_COPY(res_toZeroF, s->rtz.data(), 8 * m);
    WSV_COPY(resApprox, s->res_approx.data(), 8 * m);
    WSV_COPY(lf, s->lf.data(), 6 * n);
    WSV_COPY(HFinal, s->work.data() + (size_t)W_HF * MAX_N * MAX_N, NN);
    WSV_COPY(bFinal, s->work.data() + (size_t)W_MATS * MAX_N * MAX_N + (size_t)V_BF * MAX_N, (size_t)N);
    WSV_COPY(xAd, s->xAd.data(), (size_t)F * F * 8);
    WSV_COPY(step, s->step.data(), n);
    WSV_COPY(idepth_scaled, s->w->ids.data(), n);
    WSV_COPY(priorF, s->prior.data(), n);
#undef WSV_COPY
    if (o->frame_step) for (int i = 0; i < N; ++i) o->frame_step[i] = -s->last_x[i];
    return RC_OK;
}
// the raw accumulators and stitches of the last solve (mode 1's top words, H_L / b_L before the priors, mode 0's and the Schur's stitch)
void wsv_get_acc(HostWsv* s, double* accL, double* stL, double* stitched, double* acc) {
    const int F = s->F, N = 4 + 8 * F;
    if (accL) std::memcpy(accL, s->accL.data(), (size_t)F * F * TOP_WORDS * 8);
    if (stL) std::memcpy(stL, s->stL.data(), (size_t)N * (N + 1) * 8);
    if (stitched) std::memcpy(stitched, s->stitched.data(), (size_t)stitch_words(F) * 8);
    if (acc) std::memcpy(acc, s->acc.data(), (size_t)acc_size(F) * 8);
}
// the LDLT alone: H (N N), b (N) -> x, L (N N), d then perm (2 N)
int wsv_ldlt(int N, const double* H, const double* b, double* x, double* L, double* d_perm) {
    if (N < 1 || N > MAX_N) return RC_INVALID;
    int32_t flag[4] = {0, 0, 0, 0};
    std::vector<float> adF(2 * 64), xAd(16);
    const SolveIo io = {N, 0, 0, H, b, nullptr, adF.data(), x, xAd.data(), flag, L, d_perm};
    SolveMem* mem = new SolveMem;
    solve_serial(io, *mem);
    delete mem;
    return flag[0] ? RC_NOT_USABLE : RC_OK;
}

}  // extern "C"

#ifdef WSV_STANDALONE
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
    int H, W, F, n, m, shift;
    Params prm;
    float K[4];
    std::vector<float> images, uv, color, weights, ids, idz, energy, precalc, th, priorF, deltaF;
    std::vector<int32_t> host, point, target, state, fix, marg;
    std::vector<double> adH, adT, delta, prior, delta_prior, cPrior, cDelta, HM, bM, P;
};

Case read_case(Reader& r) {
    Case c;
    c.H = r.i32(); c.W = r.i32(); c.F = r.i32(); c.n = r.i32(); c.m = r.i32(); c.shift = r.i32();
    r.get(&c.prm, 1); r.get(c.K, 4);
    const size_t n = (size_t)c.n, m = (size_t)c.m, F = (size_t)c.F, N = 4 + 8 * F;
    c.images = r.vec<float>(F * c.H * c.W); c.host = r.vec<int32_t>(n); c.uv = r.vec<float>(2 * n); c.color = r.vec<float>(8 * n);
    c.weights = r.vec<float>(8 * n); c.ids = r.vec<float>(n); c.idz = r.vec<float>(n);
    c.point = r.vec<int32_t>(m); c.target = r.vec<int32_t>(m); c.state = r.vec<int32_t>(m); c.energy = r.vec<float>(m);
    c.precalc = r.vec<float>(F * F * 27); c.th = r.vec<float>(F); c.priorF = r.vec<float>(n); c.deltaF = r.vec<float>(n);
    c.adH = r.vec<double>(F * F * 64); c.adT = r.vec<double>(F * F * 64);
    c.delta = r.vec<double>(8 * F); c.prior = r.vec<double>(8 * F); c.delta_prior = r.vec<double>(8 * F); c.cPrior = r.vec<double>(4); c.cDelta = r.vec<double>(4);
    c.HM = r.vec<double>(N * N); c.bM = r.vec<double>(N); c.P = r.vec<double>(N * N);
    c.fix = r.vec<int32_t>(m); c.marg = r.vec<int32_t>(n);
    return c;
}

struct Run {
    HostWin* w;
    HostWsv* s;
};
Run open_case(const Case& c) {
    Run r;
    r.w = win_create(c.H, c.W, c.F);
    win_set_params(r.w, &c.prm);
    win_set_calib(r.w, c.K[0], c.K[1], c.K[2], c.K[3]);
    win_set_frames(r.w, 0, c.F, c.images.data());
    win_set_points(r.w, c.n, c.host.data(), c.uv.data(), c.color.data(), c.weights.data(), c.ids.data(), c.idz.data());
    win_set_residuals(r.w, c.m, c.point.data(), c.target.data(), c.state.data(), c.energy.data());
    r.s = wsv_create(r.w);
    return r;
}
void close_run(Run& r) { wsv_destroy(r.s); win_destroy(r.w); }
int set_state(const Case& c, Run& r) {
    return wsv_set_state(r.s, c.F, c.adH.data(), c.adT.data(), c.delta.data(), c.prior.data(), c.delta_prior.data(), c.cPrior.data(), c.cDelta.data(),
                         c.priorF.data(), c.deltaF.data());
}
void lin_apply(const Case& c, Run& r) {
    win_linearize(r.w, c.F, c.precalc.data(), c.th.data(), nullptr, nullptr);
    win_apply(r.w, 1);
}

struct Tally { long solves = 0, usable = 0, not_usable = 0, refused = 0, state = 0, margs = 0, energies = 0; };
void count(Tally& t, int rc) {
    if (rc == RC_OK) ++t.usable; else if (rc == RC_NOT_USABLE) ++t.not_usable; else if (rc == RC_INVALID) ++t.refused; else ++t.state;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    Reader rd = {std::fopen(argv[1], "rb")};
    if (!rd.f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const int ncases = rd.i32();
    Tally t;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double hostile[] = {nan, inf, -inf, 0.0, 1e30, -1e30, 1e300};
    for (int ci = 0; ci < ncases; ++ci) {
        const Case c = read_case(rd);
        const int N = 4 + 8 * c.F;
        std::vector<double> x((size_t)N), lastH((size_t)N * N), lastb((size_t)N);
        double e = 0.0;
        // the whole sequence: two rounds, then a marginalisation and a solve with the updated HM, bM
        {
            Run r = open_case(c);
            if (wsv_solve(r.s, 0, 0.0, 0, 1, c.HM.data(), c.bM.data(), nullptr, x.data(), nullptr, nullptr, nullptr) != RC_STATE) return 3;
            lin_apply(c, r);
            if (set_state(c, r) != RC_OK) return 4;
            if (wsv_step_idepths(r.s, 1.0f) != RC_STATE) return 5;
            wsv_fix_linearization(r.s, c.fix.data());
            std::vector<double> HM = c.HM, bM = c.bM;
            const int modes[] = {SOLVER_FIX_LAMBDA | SOLVER_ORTHOGONALIZE_X_LATER, SOLVER_USE_GN | SOLVER_ORTHOGONALIZE_SYSTEM, SOLVER_ORTHOGONALIZE_SYSTEM | SOLVER_ORTHOGONALIZE_X, 0};
            for (int rnd = 0; rnd < 4; ++rnd) {
                wsv_backup_idepths(r.s);
                ++t.solves;
                count(t, wsv_solve(r.s, rnd == 1 ? 2 : 0, 0.3, modes[rnd], rnd != 2, HM.data(), bM.data(), c.P.data(), x.data(), lastH.data(), lastb.data(), nullptr));
                wsv_l_energy(r.s, &e); wsv_m_energy(r.s, HM.data(), bM.data(), &e); t.energies += 2;
                wsv_step_idepths(r.s, rnd ? 0.25f : 1.0f);
                lin_apply(c, r);
            }
            // a flagged point with an active residual that is not linearized is refused; then fix every residual and marginalise
            std::vector<int32_t> all((size_t)c.m, 1), every((size_t)c.n, 1);
            const int rc0 = wsv_marginalize_points(r.s, every.data(), 1.0f, 1.0, HM.data(), bM.data(), nullptr);
            if (rc0 == RC_STATE) ++t.state;
            wsv_fix_linearization(r.s, all.data());
            int32_t res_m = 0;
            if (wsv_marginalize_points(r.s, c.marg.data(), 0.5f, 0.75, HM.data(), bM.data(), &res_m) != RC_OK) return 6;
            ++t.margs;
            ++t.solves;
            count(t, wsv_solve(r.s, 0, 0.0, SOLVER_FIX_LAMBDA, 1, HM.data(), bM.data(), nullptr, x.data(), nullptr, nullptr, nullptr));   // every residual linearized
            close_run(r);
        }
        // a refused mode bit, every hostile value in every input
        {
            Run r = open_case(c);
            lin_apply(c, r);
            set_state(c, r);
            const int bad_modes[] = {SOLVER_SVD, SOLVER_SVD_CUT7, SOLVER_MOMENTUM, SOLVER_STEPMOMENTUM, SOLVER_ORTHOGONALIZE_POINTMARG, SOLVER_ORTHOGONALIZE_FULL, 4096};
            for (int bm : bad_modes) { const int rc = wsv_solve(r.s, 0, 0.0, bm, 1, c.HM.data(), c.bM.data(), nullptr, x.data(), nullptr, nullptr, nullptr); if (rc != RC_INVALID) return 7; ++t.refused; }
            for (double v : hostile) {
                std::vector<double> HM = c.HM, bM = c.bM, P = c.P;
                HM[(size_t)N + 1] = v;
                ++t.solves; count(t, wsv_solve(r.s, 0, 0.0, 0, 1, HM.data(), c.bM.data(), nullptr, x.data(), nullptr, nullptr, nullptr));
                std::fill(HM.begin(), HM.end(), v);
                ++t.solves; count(t, wsv_solve(r.s, 0, 0.0, 0, 1, HM.data(), c.bM.data(), nullptr, x.data(), nullptr, nullptr, nullptr));
                bM[0] = v;
                ++t.solves; count(t, wsv_solve(r.s, 0, 0.0, 0, 1, c.HM.data(), bM.data(), nullptr, x.data(), nullptr, nullptr, nullptr));
                wsv_m_energy(r.s, HM.data(), bM.data(), &e); ++t.energies;
                std::fill(P.begin(), P.end(), v);
                ++t.solves; count(t, wsv_solve(r.s, 0, 0.0, SOLVER_ORTHOGONALIZE_X | SOLVER_ORTHOGONALIZE_SYSTEM, 0, c.HM.data(), c.bM.data(), P.data(), x.data(), nullptr, nullptr, nullptr));
                // priors, deltas and adjoints
                for (int which = 0; which < 7; ++which) {
                    Case d = c;
                    std::vector<double>* arr[] = {&d.adH, &d.adT, &d.delta, &d.prior, &d.delta_prior, &d.cPrior, &d.cDelta};
                    std::fill(arr[which]->begin(), arr[which]->end(), v);
                    Run q = open_case(d);
                    lin_apply(d, q);
                    const int rc = set_state(d, q);
                    if (rc == RC_OK) {
                        std::vector<int32_t> all((size_t)d.m, 1);
                        wsv_fix_linearization(q.s, d.fix.data());
                        ++t.solves; count(t, wsv_solve(q.s, 2, 0.0, SOLVER_ORTHOGONALIZE_X_LATER, 1, d.HM.data(), d.bM.data(), d.P.data(), x.data(), nullptr, nullptr, nullptr));
                        wsv_l_energy(q.s, &e); ++t.energies;
                    } else {
                        ++t.refused;
                    }
                    close_run(q);
                }
            }
            close_run(r);
        }
        // an all-zero system: no residual is active (nothing was applied), no prior, HM = 0
        {
            Case d = c;
            std::fill(d.prior.begin(), d.prior.end(), 0.0); std::fill(d.cPrior.begin(), d.cPrior.end(), 0.0);
            std::fill(d.HM.begin(), d.HM.end(), 0.0); std::fill(d.bM.begin(), d.bM.end(), 0.0);
            Run q = open_case(d);
            set_state(d, q);
            ++t.solves;
            const int rc = wsv_solve(q.s, 0, 0.0, SOLVER_USE_GN, 1, d.HM.data(), d.bM.data(), nullptr, x.data(), nullptr, nullptr, nullptr);
            count(t, rc);
            if (rc != RC_OK) return 8;
            for (int i = 0; i < N; ++i) if (x[i] != 0.0) return 9;                   // every pivot is 0: every component is 0
            close_run(q);
        }
        // a window without points
        {
            Case d = c;
            d.n = d.m = 0;
            Run q = open_case(d);
            set_state(d, q);
            ++t.solves; count(t, wsv_solve(q.s, 0, 0.0, SOLVER_FIX_LAMBDA, 1, d.HM.data(), d.bM.data(), nullptr, x.data(), nullptr, nullptr, nullptr));
            wsv_backup_idepths(q.s); wsv_step_idepths(q.s, 1.0f); wsv_l_energy(q.s, &e); ++t.energies;
            close_run(q);
        }
    }
    std::fclose(rd.f);
    std::printf("winsolve standalone: %d cases; %ld solves, %ld usable, %ld not usable, %ld refused, %ld state errors, %ld marginalisations, %ld energies\n",
                ncases, t.solves, t.usable, t.not_usable, t.refused, t.state, t.margs, t.energies);
    return 0;
}
#endif
