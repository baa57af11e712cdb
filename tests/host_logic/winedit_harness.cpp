// csrc/eds_winedit.hpp on the CPU: the entry points of include/eds_hip_winedit.h over the HostWin / HostWsv of winsolve_harness.cpp
// (included whole), bound by tests/winedit_harness.py, and — with -DWED_STANDALONE — a program of its own that drives the dumped cases
// of tests/winsolve_harness.py through the edits plus hostile flags (for a sanitizer build; it is never loaded into python that way).
// Built with g++ -ffp-contract=off.  The order of the steps is the device's (csrc/eds_winedit.hip): keep flags, the exclusive sums,
// every row into a second set of vectors, the sets exchanged.
#ifdef WED_STANDALONE
#define WSV_STANDALONE                                          // its reader of the dumped cases; its main() becomes a function nobody calls
#define main wsv_standalone_main
#endif
#include "winsolve_harness.cpp"
#undef main

#include <functional>
#include <memory>

#include "../../slam-eds_amd/csrc/eds_winedit.hpp"
#include "../../slam-eds_amd/csrc/eds_winflag.hpp"

struct WedOut { int32_t *point, *target, *res_first, *host; float *uv, *color, *weights, *idz, *deltaF, *backup; };

namespace {

// where the last wed_insert_activated put the rows: new point row -> old row, or -2 - k for the k-th activated point; new residual row
// -> old row, or -1 for a new residual
std::vector<int32_t> g_insert_map_p, g_insert_map_r;

// the states whose rows a frame's marginalisation left in place though the state is no longer valid (eds_wsv_state::rows_live on the device)
std::vector<HostWsv*> g_rows_live;
bool rows_live(const HostWin* h, const HostWsv* s) {
    if (!s) return false;
    bool live = s->valid;
    for (const HostWsv* q : g_rows_live) live = live || q == s;
    return live && s->prior.size() == (size_t)h->n && s->lin.size() == (size_t)h->m;
}

// the columns of one table and the second set they move into
struct Mover {
    edswed::Cols narrow, wide;
    std::vector<std::function<void()>> commit;
    Mover() { edswed::cols_clear(narrow); edswed::cols_clear(wide); }
    template <class T> void add(std::vector<T>& v, int words, int rows_new, bool is_wide = false) {
        auto alt = std::make_shared<std::vector<T>>((size_t)rows_new * words * 4 / sizeof(T));
        edswed::cols_add(is_wide ? wide : narrow, v.data(), alt->data(), words);
        commit.push_back([&v, alt] { v.swap(*alt); });
    }
    void run(const int32_t* map, int rows_new) {
        edswed::gather_serial(narrow, wide, map, rows_new);
        for (auto& c : commit) c();
    }
};

int compact(HostWin* h, HostWsv* s, const int32_t* keep_p, const std::vector<int32_t>& keep_r, int32_t* removed_points, int32_t* removed_residuals) {
    const int n = h->n, m = h->m;
    const bool with_state = rows_live(h, s);
    std::vector<int32_t> excl_r((size_t)m + 1), map_r((size_t)m), excl_p((size_t)n + 1), map_p((size_t)n);
    const int m2 = edswed::scan_serial(keep_r.data(), m, excl_r.data(), map_r.data());
    const int n2 = keep_p ? edswed::scan_serial(keep_p, n, excl_p.data(), map_p.data()) : n;
    std::vector<int32_t> res_point((size_t)m2), res_first((size_t)n2 + 1);
    for (int i = 0; i < m2; ++i) res_point[i] = edswed::moved_res_point(h->res_point.data(), map_r.data(), keep_p ? excl_p.data() : nullptr, i);
    for (int q = 0; q <= n2; ++q) res_first[q] = edswed::moved_res_first(h->res_first.data(), keep_p ? map_p.data() : nullptr, excl_r.data(), q, n2, m2);
    {
        Mover mv;
        mv.add(h->res_target, 1, m2); mv.add(h->state, 1, m2); mv.add(h->new_state, 1, m2); mv.add(h->active, 1, m2);
        mv.add(h->energy, 1, m2); mv.add(h->new_energy, 1, m2); mv.add(h->new_energy_wo, 1, m2); mv.add(h->ret, 1, m2);
        mv.add(h->cp, 3, m2); mv.add(h->proj, 16, m2); mv.add(h->JpJdF, 8, m2);
        if (with_state) { mv.add(s->lin, 1, m2); mv.add(s->rtz, 8, m2); mv.add(s->res_approx, 8, m2); }
        mv.add(h->J, J_WORDS, m2, true); mv.add(h->efJ, J_WORDS, m2, true);
        mv.run(map_r.data(), m2);
    }
    if (keep_p) {
        Mover mv;
        mv.add(h->pts, (int)(sizeof(Point) / 4), n2); mv.add(h->ids, 1, n2); mv.add(h->idz, 1, n2); mv.add(h->pout, (int)(sizeof(PointOut) / 4), n2);
        if (with_state) { mv.add(s->prior, 1, n2); mv.add(s->delta, 1, n2); mv.add(s->lf, 6, n2); mv.add(s->step, 1, n2); mv.add(s->backup, 1, n2); }
        mv.run(map_p.data(), n2);
    }
    h->res_point.swap(res_point); h->res_first.swap(res_first);
    h->n = n2; h->m = m2;
    if (removed_points) *removed_points = n - n2;
    if (removed_residuals) *removed_residuals = m - m2;
    return RC_OK;
}

}  // namespace

extern "C" {

int wed_remove_residuals(HostWin* h, HostWsv* s, const int32_t* select, int32_t* removed) {
    if (!h) return RC_INVALID;
    std::vector<int32_t> keep_r((size_t)h->m);
    for (int r = 0; r < h->m; ++r) keep_r[r] = edswed::keep_residual(select, h->state.data(), r);
    return compact(h, s, nullptr, keep_r, nullptr, removed);
}

int wed_remove_points(HostWin* h, HostWsv* s, const int32_t* flag, int32_t* removed_points, int32_t* removed_residuals) {
    if (!h || (!flag && h->n)) return RC_INVALID;
    std::vector<int32_t> keep_p((size_t)h->n), keep_r((size_t)h->m);
    for (int p = 0; p < h->n; ++p) keep_p[p] = edswed::keep_point(flag, p);
    for (int r = 0; r < h->m; ++r) keep_r[r] = edswed::keep_residual_of(keep_p.data(), h->res_point.data(), r);
    return compact(h, s, keep_p.data(), keep_r, removed_points, removed_residuals);
}

// marginalizeFrame's arithmetic alone: HM (N N), bM (N), prior, delta_prior (8) -> HM_out (nd nd), bM_out (nd); they may alias
int wed_marg_arith(int N, int frame, const double* HM, const double* bM, const double* prior, const double* delta_prior, double* HM_out, double* bM_out) {
    if (N < 4 + 8 * 3 || N > edswed::MAX_N || (N - 4) % 8 || frame < 0 || frame >= (N - 4) / 8) return RC_INVALID;
    if (!fin(HM, (size_t)N * N) || !fin(bM, (size_t)N) || !fin(prior, 8) || !fin(delta_prior, 8)) return RC_INVALID;
    const int nd = N - 8;
    std::vector<double> out((size_t)nd * (nd + 1));
    int32_t flag = 0;
    const edswed::MargIo io = {N, frame, HM, bM, prior, delta_prior, out.data(), out.data() + (size_t)nd * nd, &flag};
    edswed::MargMem* mem = new edswed::MargMem;
    edswed::marg_frame_serial(io, *mem);
    delete mem;
    if (flag) return RC_NOT_USABLE;
    std::memcpy(HM_out, out.data(), (size_t)nd * nd * 8);
    std::memcpy(bM_out, out.data() + (size_t)nd * nd, (size_t)nd * 8);
    return RC_OK;
}
int wed_inverse8(const double* a, double* hpi) {
    double lu[64];
    std::memcpy(lu, a, sizeof(lu));
    return edswed::inverse8(lu, hpi) ? RC_OK : RC_NOT_USABLE;
}

int wed_marginalize_frame(HostWin* h, HostWsv* s, int frame, const double* prior, const double* delta_prior, const double* HM, const double* bM,
                          double* HM_out, double* bM_out) {
    if (!h) return RC_INVALID;
    if (!prior || !delta_prior || !HM || !bM || !HM_out || !bM_out) return RC_INVALID;
    if (!s || !s->valid) return RC_STATE;
    const int F = s->F, N = 4 + 8 * F;
    if (F < 3 || F > MAX_FRAMES || frame < 0 || frame >= F) return RC_INVALID;
    if (!fin(HM, (size_t)N * N) || !fin(bM, (size_t)N) || !fin(prior, 8) || !fin(delta_prior, 8)) return RC_INVALID;
    for (int p = 0; p < h->n; ++p) if (h->pts[p].host == frame) return RC_STATE;
    if (int rc = wed_marg_arith(N, frame, HM, bM, prior, delta_prior, HM_out, bM_out)) return rc;
    std::vector<int32_t> keep_r((size_t)h->m);
    for (int r = 0; r < h->m; ++r) keep_r[r] = edswed::keep_residual_not_towards(h->res_target.data(), frame, r);
    compact(h, s, nullptr, keep_r, nullptr, nullptr);
    for (int p = 0; p < h->n; ++p) h->pts[p].host = edswed::frame_after(h->pts[p].host, frame);
    for (int r = 0; r < h->m; ++r) h->res_target[r] = edswed::frame_after(h->res_target[r], frame);
    const size_t px = (size_t)h->H * h->W;
    for (int f = frame + 1; f < F; ++f) std::memcpy(h->frames.data() + (size_t)(f - 1) * px, h->frames.data() + (size_t)f * px, px * sizeof(Px));
    s->valid = false; s->lf_on = false; s->have_backup = s->have_step = s->have_system = false;
    g_rows_live.push_back(s);
    return RC_OK;
}

int wed_set_state(HostWin* h, HostWsv* s, int F, const double* adHost, const double* adTarget, const double* delta, const double* prior,
                  const double* delta_prior, const double* cPrior, const double* cDelta) {
    if (!h || !s) return RC_INVALID;
    const bool live = rows_live(h, s);
    for (size_t k = 0; k < g_rows_live.size(); ++k)
        if (g_rows_live[k] == s) { g_rows_live.erase(g_rows_live.begin() + k); break; }
    const std::vector<float> prior_f = s->prior, rtz = s->rtz;
    const std::vector<int32_t> lin = s->lin;
    std::vector<float> delta_f((size_t)h->n);
    for (int p = 0; p < h->n; ++p) delta_f[p] = delta_of_idepths(h->ids[p], h->idz[p], h->s.scale_idepth);
    if (int rc = wsv_set_state(s, F, adHost, adTarget, delta, prior, delta_prior, cPrior, cDelta, live ? prior_f.data() : nullptr, delta_f.data())) return rc;
    if (live) { s->lin = lin; s->rtz = rtz; }
    return RC_OK;
}

// eds_wed_insert_activated from the arrays eds_act_get_activated returns (K points of hosts `host`, indices `index` below mp, F hosts);
// cap_points / cap_residuals: the window's capacity (the host window has none of its own)
int wed_insert_activated(HostWin* h, HostWsv* s, int F, int mp, int K, const int32_t* host, const int32_t* index, const float* uv, const float* color,
                         const float* weights, const float* idepth, const uint64_t* mask, int cap_points, int cap_residuals, int32_t* inserted_points,
                         int32_t* inserted_residuals) {
    if (!h || F < 2 || F > MAX_FRAMES || mp < 1 || K < 0) return RC_INVALID;
    for (int p = 0; p < h->n; ++p) if (h->pts[p].host >= F) return RC_INVALID;
    const size_t C = (size_t)F * mp, G = C * F;
    const int n = h->n, m = h->m;
    std::vector<int32_t> keep_c(C, 0), keep_g(G, 0), excl_c(C + 1), excl_g(G + 1), map_c(C), map_g(G), first(9, n);
    std::vector<int> list_of(C, -1);
    for (int k = 0; k < K; ++k) {
        if (host[k] < 0 || host[k] >= F || index[k] < 0 || index[k] >= mp) return RC_INVALID;
        const size_t c = (size_t)host[k] * mp + index[k];
        keep_c[c] = 1; list_of[c] = k;
        for (int t = 0; t < F; ++t) keep_g[c * F + t] = (int32_t)(mask[k] >> t & 1u);
    }
    edswed::scan_serial(keep_c.data(), (int)C, excl_c.data(), map_c.data());
    const int R = edswed::scan_serial(keep_g.data(), (int)G, excl_g.data(), map_g.data());
    const int n2 = n + K, m2 = m + R;
    if (n2 > cap_points || m2 > cap_residuals) return RC_STATE;
    for (int f = 0, p = 0; f < 9; ++f) { first[f] = p; while (p < n && h->pts[p].host == f) ++p; }
    const edswed::Ins si = {F, mp, first.data(), h->res_first.data(), excl_c.data(), excl_g.data()};
    std::vector<int32_t> map_p((size_t)n2, -1), map_r((size_t)m2, -1), res_point((size_t)m2), res_first((size_t)n2 + 1);
    for (int p = 0; p < n; ++p) {
        const int q = edswed::ins_old_point(si, p, h->pts[p].host);
        map_p[q] = p; res_first[q] = edswed::ins_old_res(si, h->res_first[p], h->pts[p].host);
    }
    for (int r = 0; r < m; ++r) {
        const int p = h->res_point[r], hh = h->pts[p].host, i = edswed::ins_old_res(si, r, hh);
        map_r[i] = r; res_point[i] = edswed::ins_old_point(si, p, hh);
    }
    const bool with_state = rows_live(h, s);
    {
        Mover mv;
        mv.add(h->res_target, 1, m2); mv.add(h->state, 1, m2); mv.add(h->new_state, 1, m2); mv.add(h->active, 1, m2);
        mv.add(h->energy, 1, m2); mv.add(h->new_energy, 1, m2); mv.add(h->new_energy_wo, 1, m2); mv.add(h->ret, 1, m2);
        mv.add(h->cp, 3, m2); mv.add(h->proj, 16, m2); mv.add(h->JpJdF, 8, m2);
        if (with_state) { mv.add(s->lin, 1, m2); mv.add(s->rtz, 8, m2); mv.add(s->res_approx, 8, m2); }
        mv.add(h->J, J_WORDS, m2, true); mv.add(h->efJ, J_WORDS, m2, true);
        mv.run(map_r.data(), m2);
    }
    {
        Mover mv;
        mv.add(h->pts, (int)(sizeof(Point) / 4), n2); mv.add(h->ids, 1, n2); mv.add(h->idz, 1, n2); mv.add(h->pout, (int)(sizeof(PointOut) / 4), n2);
        if (with_state) { mv.add(s->prior, 1, n2); mv.add(s->delta, 1, n2); mv.add(s->lf, 6, n2); mv.add(s->step, 1, n2); mv.add(s->backup, 1, n2); }
        mv.run(map_p.data(), n2);
    }
    for (int kk = 0; kk < K; ++kk) {                              // in (host, index) order: map_c
        const int c = map_c[kk], k = list_of[c], q = edswed::ins_new_point(si, c);
        Point& o = h->pts[q];
        o.host = c / mp; o.u = uv[2 * k]; o.v = uv[2 * k + 1];
        for (int j = 0; j < 8; ++j) { o.color[j] = color[8 * k + j]; o.weights[j] = weights[8 * k + j]; }
        h->ids[q] = h->idz[q] = idepth[k];
        res_first[q] = edswed::ins_new_res(si, (int64_t)c * F);
        map_p[q] = -2 - k;
    }
    g_insert_map_p = map_p; g_insert_map_r = map_r;
    for (int j = 0; j < R; ++j) {
        const int64_t g = map_g[j];
        const int r = edswed::ins_new_res(si, g);
        res_point[r] = edswed::ins_new_point(si, (int)(g / F)); h->res_target[r] = (int)(g % F); h->new_state[r] = ST_OUTLIER;
    }
    res_first[n2] = m2;
    h->res_point.swap(res_point); h->res_first.swap(res_first);
    h->n = n2; h->m = m2;
    if (inserted_points) *inserted_points = K;
    if (inserted_residuals) *inserted_residuals = R;
    return RC_OK;
}

// eds_wfl_insert_frame_residuals over the window's rows (the history's columns are tests/winflag_harness.py's): every point not hosted by
// `frame` and without a residual towards it gets one at the end of its run, as eds_win_set_residuals leaves state IN and energy 0
int wed_insert_frame_residuals(HostWin* h, HostWsv* s, int frame, int cap_residuals, int32_t* inserted) {
    if (!h || frame < 0 || frame >= h->max_frames) return RC_INVALID;
    const int n = h->n, m = h->m;
    std::vector<int32_t> need((size_t)n + 1, 0), excl((size_t)n + 1), map_p((size_t)n + 1);
    for (int p = 0; p < n; ++p) need[p] = edswfl::needs_residual(h->res_first.data(), h->res_target.data(), h->pts[p].host, p, frame);
    const int K = edswed::scan_serial(need.data(), n, excl.data(), map_p.data());
    const int m2 = m + K;
    if (m2 > cap_residuals) return RC_STATE;
    if (inserted) *inserted = K;
    if (!K) return RC_OK;
    std::vector<int32_t> map_r((size_t)m2, -1), res_point((size_t)m2), res_first((size_t)n + 1);
    for (int r = 0; r < m; ++r) {
        const int p = h->res_point[r], i = edswfl::moved_row(excl.data(), p, r);
        map_r[i] = r; res_point[i] = p;
    }
    for (int q = 0; q <= n; ++q) res_first[q] = edswfl::moved_first(h->res_first.data(), excl.data(), q);
    const bool with_state = rows_live(h, s);
    {
        Mover mv;
        mv.add(h->res_target, 1, m2); mv.add(h->state, 1, m2); mv.add(h->new_state, 1, m2); mv.add(h->active, 1, m2);
        mv.add(h->energy, 1, m2); mv.add(h->new_energy, 1, m2); mv.add(h->new_energy_wo, 1, m2); mv.add(h->ret, 1, m2);
        mv.add(h->cp, 3, m2); mv.add(h->proj, 16, m2); mv.add(h->JpJdF, 8, m2);
        if (with_state) { mv.add(s->lin, 1, m2); mv.add(s->rtz, 8, m2); mv.add(s->res_approx, 8, m2); }
        mv.add(h->J, J_WORDS, m2, true); mv.add(h->efJ, J_WORDS, m2, true);
        mv.run(map_r.data(), m2);
    }
    for (int p = 0; p < n; ++p) {
        if (!need[p]) continue;
        const int r = edswfl::new_row(h->res_first.data(), excl.data(), p);
        res_point[r] = p; h->res_target[r] = frame; h->new_state[r] = ST_OUTLIER;
    }
    h->res_point.swap(res_point); h->res_first.swap(res_first);
    h->m = m2;
    return RC_OK;
}

// eds_wfl_flag_points' resetOOB: every residual of a point with mask[p] != 0 (the linearize, apply and fix that follow are the window's
// and the solver's own functions over those points)
int wed_reset_oob(HostWin* h, HostWsv* s, const int32_t* mask) {
    if (!h || !s || (!mask && h->n)) return RC_INVALID;
    if (!s->valid) return RC_STATE;
    for (int r = 0; r < h->m; ++r)
        if (mask[h->res_point[r]]) edswfl::reset_oob(r, h->state.data(), h->new_state.data(), h->energy.data(), h->new_energy.data(), s->lin.data());
    return RC_OK;
}

// the maps of the last wed_insert_activated (n and m as it left them)
int wed_last_insert_maps(int n, int m, int32_t* map_p, int32_t* map_r) {
    if ((size_t)n != g_insert_map_p.size() || (size_t)m != g_insert_map_r.size()) return RC_STATE;
    if (n) std::memcpy(map_p, g_insert_map_p.data(), (size_t)n * 4);
    if (m) std::memcpy(map_r, g_insert_map_r.data(), (size_t)m * 4);
    return RC_OK;
}

// a solver that is about to be used anew (or has been closed) is in no list: its address may be an earlier solver's
void wed_forget(HostWsv* s) {
    for (size_t k = 0; k < g_rows_live.size();)
        if (g_rows_live[k] == s) g_rows_live.erase(g_rows_live.begin() + k); else ++k;
}

int wed_counts(HostWin* h, int32_t* n, int32_t* m, int32_t* per_host) {
    if (!h) return RC_INVALID;
    if (n) *n = h->n;
    if (m) *m = h->m;
    if (per_host) {
        std::vector<int32_t> host_of((size_t)h->n);
        for (int p = 0; p < h->n; ++p) host_of[p] = h->pts[p].host;
        edswed::per_host_counts(host_of, per_host);
    }
    return RC_OK;
}

// the window's host copies after an edit, from the same flags (what the device entry points keep beside the tables)
int wed_edit_mirrors(int n, int m, int32_t* host_of, int32_t* point, int32_t* target, const int32_t* keep_p, const int32_t* keep_r, int32_t* out4) {
    edswed::Mirrors w;
    w.n = n; w.m = m;
    w.host_of.assign(host_of, host_of + n); w.point.assign(point, point + m); w.target.assign(target, target + m);
    edswed::edit_mirrors(w, keep_p, keep_r);
    std::memcpy(host_of, w.host_of.data(), (size_t)w.n * 4); std::memcpy(point, w.point.data(), (size_t)w.m * 4); std::memcpy(target, w.target.data(), (size_t)w.m * 4);
    out4[0] = w.n; out4[1] = w.m; out4[2] = w.max_host; out4[3] = w.max_target;
    return RC_OK;
}

int wed_get(HostWin* h, HostWsv* s, const WedOut* o) {
    if (!h || !o) return RC_INVALID;
    if (o->backup && !(s && s->valid)) return RC_STATE;
    const size_t n = (size_t)h->n, m = (size_t)h->m;
    if (o->point && m) std::memcpy(o->point, h->res_point.data(), m * 4);
    if (o->target && m) std::memcpy(o->target, h->res_target.data(), m * 4);
    if (o->res_first) std::memcpy(o->res_first, h->res_first.data(), (n + 1) * 4);
    if (o->idz && n) std::memcpy(o->idz, h->idz.data(), n * 4);
    if (o->deltaF && n && rows_live(h, s) && s->delta.size() == n) std::memcpy(o->deltaF, s->delta.data(), n * 4);   // as on the device: the row outlives a frame's marginalisation
    if (o->backup && n) { if (s->have_backup) std::memcpy(o->backup, s->backup.data(), n * 4); else std::memset(o->backup, 0, n * 4); }
    for (size_t i = 0; i < n; ++i) {
        const Point& p = h->pts[i];
        if (o->host) o->host[i] = p.host;
        if (o->uv) { o->uv[2 * i] = p.u; o->uv[2 * i + 1] = p.v; }
        if (o->color) std::memcpy(o->color + 8 * i, p.color, 32);
        if (o->weights) std::memcpy(o->weights + 8 * i, p.weights, 32);
    }
    return RC_OK;
}

}  // extern "C"

#ifdef WED_STANDALONE
namespace {

// the grouping eds_hip_window.h asks for, and every table as long as the counts say
bool consistent(const HostWin* h, const HostWsv* s) {
    const size_t n = (size_t)h->n, m = (size_t)h->m;
    if (h->pts.size() != n || h->ids.size() != n || h->idz.size() != n || h->pout.size() != n || h->res_first.size() != n + 1) return false;
    if (h->res_point.size() != m || h->res_target.size() != m || h->J.size() != m * J_WORDS || h->efJ.size() != m * J_WORDS || h->proj.size() != m * 16) return false;
    if (s->valid && (s->lin.size() != m || s->rtz.size() != m * 8 || s->prior.size() != n || s->lf.size() != n * 6 || s->backup.size() != n)) return false;
    if (h->res_first[0] != 0 || h->res_first[n] != (int)m) return false;
    for (size_t p = 0; p < n; ++p) {
        if (h->res_first[p] > h->res_first[p + 1]) return false;
        for (int r = h->res_first[p]; r < h->res_first[p + 1]; ++r) if (h->res_point[r] != (int)p) return false;
        if (p && h->pts[p].host < h->pts[p - 1].host) return false;
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    Reader rd = {std::fopen(argv[1], "rb")};
    if (!rd.f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const int ncases = rd.i32();
    long edits = 0, solves = 0, rows_removed = 0, frames_marginalised = 0, refused = 0, not_usable = 0, inserts = 0, over_capacity = 0;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double hostile[] = {nan, inf, -inf};           // 1e300 is finite: it runs, and ends not usable
    for (int ci = 0; ci < ncases; ++ci) {
        const Case c = read_case(rd);
        const int N = 4 + 8 * c.F;
        std::vector<double> x((size_t)N);
        // flag patterns: none, every third, the first and the last, one whole host, hostile values (any nonzero word is a flag), all
        for (int pattern = 0; pattern < 6; ++pattern) {
            Run r = open_case(c);
            lin_apply(c, r);
            if (set_state(c, r) != RC_OK) return 3;
            wsv_fix_linearization(r.s, c.fix.data());
            wsv_backup_idepths(r.s);
            wsv_solve(r.s, 0, 0.0, SOLVER_FIX_LAMBDA, 1, c.HM.data(), c.bM.data(), nullptr, x.data(), nullptr, nullptr, nullptr); ++solves;
            std::vector<int32_t> pf((size_t)c.n, 0), rf((size_t)c.m, 0);
            for (int p = 0; p < c.n; ++p) {
                const bool on = pattern == 1 ? p % 3 == 0 : pattern == 2 ? (p == 0 || p == c.n - 1) : pattern == 3 ? c.host[p] == c.host[0] : pattern >= 4;
                pf[p] = on ? (pattern == 4 ? (p % 2 ? INT32_MIN : -1) : 1) : 0;
            }
            for (int q = 0; q < c.m; ++q) rf[q] = pattern == 0 ? 0 : pattern == 5 ? 1 : (q * 7 + pattern) % 4 == 0 ? INT32_MAX : 0;
            int32_t a = 0, b = 0, e = 0;
            if (wed_remove_residuals(r.w, r.s, rf.data(), &a) != RC_OK || !consistent(r.w, r.s)) return 4;
            if (wed_remove_residuals(r.w, r.s, nullptr, &e) != RC_OK || !consistent(r.w, r.s)) return 5;
            for (int q = 0; q < r.w->m; ++q) if (r.w->state[q] != ST_IN) return 6;
            if (wed_remove_points(r.w, r.s, pf.data(), &b, &e) != RC_OK || !consistent(r.w, r.s)) return 7;
            if (pattern >= 4 && (r.w->n || r.w->m)) return 8;
            if (pattern == 0 && (a || b || r.w->n != c.n)) return 9;
            edits += 3; rows_removed += a + b + e;
            // the window goes on: another round over what is left, an empty window included
            lin_apply(c, r);
            wsv_solve(r.s, 0, 0.0, SOLVER_FIX_LAMBDA, 1, c.HM.data(), c.bM.data(), nullptr, x.data(), nullptr, nullptr, nullptr); ++solves;
            wsv_step_idepths(r.s, 1.0f);
            // ... and an edit of the edited window, with no flags at all
            std::vector<int32_t> none((size_t)r.w->n, 0);
            if (wed_remove_points(r.w, r.s, none.data(), &b, &e) != RC_OK || b || e || !consistent(r.w, r.s)) return 10;
            ++edits;
            close_run(r);
        }
        // before any eds_wsv state: the window's own rows only
        {
            Run r = open_case(c);
            lin_apply(c, r);
            std::vector<int32_t> pf((size_t)c.n, 0);
            for (int p = 0; p < c.n; p += 2) pf[p] = 1;
            int32_t b = 0, e = 0;
            if (wed_remove_points(r.w, r.s, pf.data(), &b, &e) != RC_OK || !consistent(r.w, r.s) || b != (c.n + 1) / 2) return 11;
            if (wed_remove_points(r.w, r.s, nullptr, &b, &e) != (r.w->n ? RC_INVALID : RC_OK)) return 12;
            ++edits;
            close_run(r);
        }
        // activated points enter: a made-up fit of three points a host (every other frame IN), capacity exceeded, indices outside, all flags set
        {
            Run r = open_case(c);
            lin_apply(c, r);
            if (set_state(c, r) != RC_OK) return 31;
            wsv_fix_linearization(r.s, c.fix.data());
            const int mp = 5, K = 3 * c.F;
            std::vector<int32_t> ah((size_t)K), ai((size_t)K);
            std::vector<float> auv(2 * (size_t)K, 9.0f), acol(8 * (size_t)K, 100.0f), aw(8 * (size_t)K, 0.75f), aid((size_t)K, 0.5f);
            std::vector<uint64_t> mask((size_t)K);
            int R = 0;
            for (int k = 0; k < K; ++k) {
                ah[k] = k / 3; ai[k] = (k % 3) * 2;
                mask[k] = (((uint64_t)1 << c.F) - 1) & ~((uint64_t)1 << ah[k]);
                R += c.F - 1;
            }
            int32_t ip = 0, ir = 0;
            const int n0 = r.w->n, m0 = r.w->m;
            if (wed_insert_activated(r.w, r.s, c.F, mp, K, ah.data(), ai.data(), auv.data(), acol.data(), aw.data(), aid.data(), mask.data(), n0 + K - 1, m0 + R, &ip, &ir) != RC_STATE) return 32;
            if (wed_insert_activated(r.w, r.s, c.F, mp, K, ah.data(), ai.data(), auv.data(), acol.data(), aw.data(), aid.data(), mask.data(), n0 + K, m0 + R - 1, &ip, &ir) != RC_STATE) return 33;
            over_capacity += 2;
            if (r.w->n != n0 || r.w->m != m0 || !consistent(r.w, r.s)) return 34;
            ai[0] = mp;
            if (wed_insert_activated(r.w, r.s, c.F, mp, K, ah.data(), ai.data(), auv.data(), acol.data(), aw.data(), aid.data(), mask.data(), 1 << 22, 1 << 24, &ip, &ir) != RC_INVALID) return 35;
            ai[0] = 0;
            if (wed_insert_activated(r.w, r.s, c.F, mp, K, ah.data(), ai.data(), auv.data(), acol.data(), aw.data(), aid.data(), mask.data(), n0 + K, m0 + R, &ip, &ir) != RC_OK) return 36;
            if (ip != K || ir != R || r.w->n != n0 + K || !consistent(r.w, r.s)) return 37;
            ++inserts;
            lin_apply(c, r);
            std::vector<int32_t> every((size_t)r.w->n, 1);
            if (wed_remove_points(r.w, r.s, every.data(), nullptr, nullptr) != RC_OK || r.w->n) return 38;
            if (wed_insert_activated(r.w, r.s, c.F, mp, K, ah.data(), ai.data(), auv.data(), acol.data(), aw.data(), aid.data(), mask.data(), K, R, &ip, &ir) != RC_OK) return 39;   // into an empty window
            if (!consistent(r.w, r.s)) return 40;
            ++inserts;
            close_run(r);
        }
        // frames leave one after the other until two are left; hostile values, a hosted point and an empty window on the way
        if (c.F >= 3) {
            Run r = open_case(c);
            lin_apply(c, r);
            if (set_state(c, r) != RC_OK) return 13;
            wsv_fix_linearization(r.s, c.fix.data());
            int F = c.F;
            std::vector<double> HM = c.HM, bM = c.bM, adH = c.adH, adT = c.adT, delta = c.delta, prior = c.prior, dprior = c.delta_prior;
            std::vector<float> precalc = c.precalc, th = c.th;
            while (F > 2) {
                const int N2 = 4 + 8 * F, frame = F == c.F ? 0 : F / 2;
                const double* pr = prior.data() + 8 * frame;
                const double* dp = dprior.data() + 8 * frame;
                std::vector<double> h2((size_t)(N2 - 8) * (N2 - 8)), b2((size_t)N2 - 8);
                bool hosted = false;
                for (int p = 0; p < r.w->n; ++p) hosted = hosted || r.w->pts[p].host == frame;
                if (hosted && wed_marginalize_frame(r.w, r.s, frame, pr, dp, HM.data(), bM.data(), h2.data(), b2.data()) != RC_STATE) return 14;
                refused += hosted;
                std::vector<int32_t> pf((size_t)r.w->n);
                for (int p = 0; p < r.w->n; ++p) pf[p] = r.w->pts[p].host == frame;
                if (wed_remove_points(r.w, r.s, pf.data(), nullptr, nullptr) != RC_OK) return 15;
                for (double v : hostile) {
                    std::vector<double> hh = HM, bb = bM, pp(pr, pr + 8), dd(dp, dp + 8);
                    hh[(size_t)N2 + 1] = v;
                    if (wed_marginalize_frame(r.w, r.s, frame, pr, dp, hh.data(), bM.data(), h2.data(), b2.data()) != RC_INVALID) return 16;
                    bb[0] = v;
                    if (wed_marginalize_frame(r.w, r.s, frame, pr, dp, HM.data(), bb.data(), h2.data(), b2.data()) != RC_INVALID) return 17;
                    pp[3] = v; dd[5] = v;
                    if (wed_marginalize_frame(r.w, r.s, frame, pp.data(), dp, HM.data(), bM.data(), h2.data(), b2.data()) != RC_INVALID) return 18;
                    if (wed_marginalize_frame(r.w, r.s, frame, pr, dd.data(), HM.data(), bM.data(), h2.data(), b2.data()) != RC_INVALID) return 19;
                    refused += 4;
                }
                {   // finite, and the arithmetic overflows or meets a zero block: not usable, nothing changes
                    std::vector<double> hh(HM.size(), 1e300), zero(8, 0.0), hz = HM;
                    const int m_before = r.w->m;
                    int rc = wed_marginalize_frame(r.w, r.s, frame, pr, dp, hh.data(), bM.data(), h2.data(), b2.data());
                    if (rc != RC_NOT_USABLE && rc != RC_OK) return 20;
                    if (rc == RC_OK) return 21;                 // S^2 overflows: every scaled entry is 0
                    const int io = 4 + 8 * frame;
                    for (int i = 0; i < N2; ++i) for (int k = 0; k < 8; ++k) hz[(size_t)i * N2 + io + k] = hz[(size_t)(io + k) * N2 + i] = 0.0;
                    if (wed_marginalize_frame(r.w, r.s, frame, zero.data(), zero.data(), hz.data(), bM.data(), h2.data(), b2.data()) != RC_NOT_USABLE) return 22;
                    if (r.w->m != m_before || !r.s->valid) return 23;
                    not_usable += 2;
                }
                if (wed_marginalize_frame(r.w, r.s, frame, pr, dp, HM.data(), bM.data(), h2.data(), b2.data()) != RC_OK || !consistent(r.w, r.s)) return 24;
                ++frames_marginalised;
                if (wed_marginalize_frame(r.w, r.s, 0, pr, dp, h2.data(), b2.data(), h2.data(), b2.data()) != RC_STATE) return 25;   // no valid state now
                ++refused;
                // the caller's per-frame inputs without the frame
                std::vector<double> a2, t2, d2, p2, q2;
                std::vector<float> pc2, th2;
                for (int t = 0; t < F; ++t)
                    for (int hh = 0; hh < F; ++hh) {
                        if (t == frame || hh == frame) continue;
                        a2.insert(a2.end(), adH.begin() + 64 * (hh + F * t), adH.begin() + 64 * (hh + F * t) + 64);
                        t2.insert(t2.end(), adT.begin() + 64 * (hh + F * t), adT.begin() + 64 * (hh + F * t) + 64);
                        pc2.insert(pc2.end(), precalc.begin() + 27 * (t + F * hh), precalc.begin() + 27 * (t + F * hh) + 27);
                    }
                for (int f = 0; f < F; ++f) {
                    if (f == frame) continue;
                    d2.insert(d2.end(), delta.begin() + 8 * f, delta.begin() + 8 * f + 8); p2.insert(p2.end(), prior.begin() + 8 * f, prior.begin() + 8 * f + 8);
                    q2.insert(q2.end(), dprior.begin() + 8 * f, dprior.begin() + 8 * f + 8); th2.push_back(th[f]);
                }
                // precalc is [h F + t]: the loop above walked t outside, so transpose the pairs back
                std::vector<float> pc3(pc2.size());
                for (int t = 0; t < F - 1; ++t) for (int hh = 0; hh < F - 1; ++hh) std::memcpy(pc3.data() + 27 * (hh * (F - 1) + t), pc2.data() + 27 * (t * (F - 1) + hh), 27 * 4);
                adH = a2; adT = t2; delta = d2; prior = p2; dprior = q2; th = th2; precalc = pc3; HM = h2; bM = b2;
                --F;
                if (wed_set_state(r.w, r.s, F, adH.data(), adT.data(), delta.data(), prior.data(), dprior.data(), c.cPrior.data(), c.cDelta.data()) != RC_OK) return 26;
                win_linearize(r.w, F, precalc.data(), th.data(), nullptr, nullptr);
                win_apply(r.w, 1);
                std::vector<double> x2((size_t)4 + 8 * F);
                wsv_backup_idepths(r.s);
                wsv_solve(r.s, 0, 0.0, SOLVER_FIX_LAMBDA, 1, HM.data(), bM.data(), nullptr, x2.data(), nullptr, nullptr, nullptr); ++solves;
                wsv_step_idepths(r.s, 1.0f);
                if (!consistent(r.w, r.s)) return 27;
            }
            // two frames are left: refused; and an empty window marginalises nothing but still has its arithmetic
            std::vector<double> h2(HM.size()), b2(bM.size());
            if (wed_marginalize_frame(r.w, r.s, 0, prior.data(), dprior.data(), HM.data(), bM.data(), h2.data(), b2.data()) != RC_INVALID) return 28;
            ++refused;
            close_run(r);
            Case d = c;
            d.n = d.m = 0;
            Run q = open_case(d);
            if (set_state(d, q) != RC_OK) return 29;
            std::vector<double> h3((size_t)(N - 8) * (N - 8)), b3((size_t)N - 8);
            if (wed_marginalize_frame(q.w, q.s, c.F - 1, c.prior.data() + 8 * (c.F - 1), c.delta_prior.data() + 8 * (c.F - 1), c.HM.data(), c.bM.data(), h3.data(), b3.data()) != RC_OK) return 30;
            ++frames_marginalised;
            close_run(q);
        }
    }
    std::fclose(rd.f);
    std::printf("winedit standalone: %ld inserts, %ld refused for capacity\n", inserts, over_capacity);
    std::printf("winedit standalone: %d cases; %ld edits, %ld solves, %ld rows removed; %ld frames marginalised, %ld refused, %ld not usable\n", ncases, edits,
                solves, rows_removed, frames_marginalised, refused, not_usable);
    return 0;
}
#endif
