// csrc/eds_activate.hpp on the CPU: the entry points tests/activate_harness.py binds, and — with -DACT_STANDALONE — a program of its own
// that runs a dumped set of cases plus hostile inputs (for a sanitizer build; it is never loaded into python that way).
// Built with g++ -ffp-contract=off.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../slam-eds_amd/csrc/eds_activate.hpp"

using namespace edsact;

extern "C" {

int act_point_size(void) { return (int)sizeof(Point); }
int act_params_size(void) { return (int)sizeof(Params); }
void act_params_default(Params* p) { *p = params_default(); }
int act_params_valid(const Params* p) { return params_valid(*p) ? 1 : 0; }

// out: h1 x w1 floats
void act_make_map(int w1, int h1, int newest, const float* KRKi1, const float* Kt1, int n_active, const int32_t* active_host, const float* active,
                  uint8_t* map) {
    make_map_serial(map, w1, h1, newest, KRKi1, Kt1, n_active, active_host, active);
}

void act_map_values(const uint8_t* map, int cells, float* out) {
    for (int i = 0; i < cells; ++i) out[i] = map_value(map[i]);
}

// select_body with one thread; points: [n_hosts][max_points]
void act_select(const Point* points, int max_points, const int32_t* n, int newest, int n_hosts, const float* KRKi1, const float* Kt1,
                const uint8_t* flagged, float min_act_dist, const Params* s, int w1, int h1, uint8_t* map, int32_t* fate, int32_t* counts) {
    std::vector<uint32_t> mark((size_t)w1 * h1);
    SelectIn in = {points, max_points, n, newest, n_hosts, KRKi1, Kt1, flagged, min_act_dist, *s, w1, h1, map, mark.data(), fate, counts};
    SerialSync sync;
    select_body(in, 0, 1, sync);
}

// the gradient planes of n frames, [n][H][W] Grad
void act_gradients(const float* colors, int n, int H, int W, Grad* out) {
    const size_t px = (size_t)H * W;
    for (int f = 0; f < n; ++f)
        for (int i = 0; i < H * W; ++i) out[px * f + i] = edsimm::gradient_at(colors + px * f, W, H, i);
}

// the fit of every CHOSEN point and the retirement of what leaves; colors: [n_hosts][H][W]; grads: act_gradients' planes, or NULL to
// form them here; fit: [..][4]; res_*: [..][n_hosts]
void act_optimize_g(Point* points, int max_points, const int32_t* n, int n_hosts, const float* pre, const float* colors, const Grad* grads, int H, int W,
                    float fx, float fy, float cx, float cy, const Params* s, float huber, int32_t* fate, float* fit, int32_t* res_state,
                    float* res_energy) {
    const Calib K = make_calib(H, W, fx, fy, cx, cy);
    std::vector<Grad> own;
    if (!grads) {
        own.resize((size_t)H * W * n_hosts);
        act_gradients(colors, n_hosts, H, W, own.data());
    }
    const Grad* g_planes = grads ? grads : own.data();
    for (int h = 0; h < n_hosts; ++h)
        for (int i = 0; i < n[h]; ++i) {
            const size_t idx = (size_t)h * max_points + i;
            Point& p = points[idx];
            for (int t = 0; t < n_hosts; ++t) { res_state[idx * n_hosts + t] = -1; res_energy[idx * n_hosts + t] = 0.0f; }
            for (int k = 0; k < 4; ++k) fit[idx * 4 + k] = 0.0f;
            if (fate[idx] == CHOSEN) {
                const Fit o = fit_serial(K, *s, huber, pre, colors, g_planes, p, h, n_hosts, res_state + idx * n_hosts, res_energy + idx * n_hosts);
                fit[idx * 4] = o.idepth; fit[idx * 4 + 1] = o.E; fit[idx * 4 + 2] = o.Hdd; fit[idx * 4 + 3] = o.bd;
                fate[idx] = o.fate;
            }
            if (p.alive && leaves(fate[idx], p.status)) p.alive = 0;
        }
}

void act_optimize(Point* points, int max_points, const int32_t* n, int n_hosts, const float* pre, const float* colors, int H, int W, float fx, float fy,
                  float cx, float cy, const Params* s, float huber, int32_t* fate, float* fit, int32_t* res_state, float* res_energy) {
    act_optimize_g(points, max_points, n, n_hosts, pre, colors, nullptr, H, W, fx, fy, cx, cy, s, huber, fate, fit, res_state, res_energy);
}

}  // extern "C"

#ifdef ACT_STANDALONE
namespace {

struct Reader {
    FILE* f;
    template <class T> void get(T* p, size_t n) {
        if (n && std::fread(p, sizeof(T), n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); }
    }
    int i32() { int32_t v; get(&v, 1); return v; }
    float f32() { float v; get(&v, 1); return v; }
};

struct Case {
    int H, W, F, max_points, newest, n_active;
    Params s;
    float huber, K4[4], min_dist;
    std::vector<int32_t> n, active_host;
    std::vector<Point> points;
    std::vector<float> colors, KRKi1, Kt1, active, pre;
    std::vector<uint8_t> flagged;
};

long hist[NUM_FATES], runs, zero_cells;

void run(const Case& c, int w1, int h1) {
    std::vector<uint8_t> map((size_t)w1 * h1);
    act_make_map(w1, h1, c.newest, c.KRKi1.data(), c.Kt1.data(), c.n_active, c.active_host.data(), c.active.data(), map.data());
    std::vector<Point> pts = c.points;
    const size_t np = pts.size();
    std::vector<int32_t> fate(np, 0), rs(np * c.F);
    std::vector<float> fit(np * 4), re(np * c.F);
    int32_t counts[NUM_FATES];
    act_select(pts.data(), c.max_points, c.n.data(), c.newest, c.F, c.KRKi1.data(), c.Kt1.data(), c.flagged.data(), c.min_dist, &c.s, w1, h1, map.data(),
               fate.data(), counts);
    act_optimize(pts.data(), c.max_points, c.n.data(), c.F, c.pre.data(), c.colors.data(), c.H, c.W, c.K4[0], c.K4[1], c.K4[2], c.K4[3], &c.s, c.huber,
                 fate.data(), fit.data(), rs.data(), re.data());
    for (int h = 0; h < c.F; ++h)
        for (int i = 0; i < c.n[h]; ++i) ++hist[fate[(size_t)h * c.max_points + i]];
    for (uint8_t b : map) zero_cells += b == 0;
    ++runs;
}

// one case bent into inputs no caller should pass
void hostile(const Case& base) {
    const float nan = edsimm::nan_f(), inf = 1.0f / 0.0f;
    const float bad[] = {nan, inf, -inf, 0.0f, 1e30f};
    const int w1 = base.W >> 1, h1 = base.H >> 1;
    for (float b : bad) {
        for (int where = 0; where < 4; ++where) {
            Case c = base;
            if (where == 0) for (size_t i = 0; i < c.KRKi1.size(); i += 4) c.KRKi1[i] = b;
            if (where == 1) for (size_t i = 0; i < c.Kt1.size(); i += 2) c.Kt1[i] = b;
            if (where == 2) for (size_t i = 0; i < c.pre.size(); i += 5) c.pre[i] = b;
            if (where == 3) for (int i = 0; i < c.n_active; ++i) c.active[3 * i + 2] = b;
            run(c, w1, h1);
        }
    }
    {   // active points at +-2^31, every point on the image border, idepth_min = idepth_max = 0, gn_its 16
        Case c = base;
        for (int i = 0; i < c.n_active; ++i) { c.active[3 * i] = (i & 1) ? 2147483648.0f : -2147483648.0f; c.active[3 * i + 1] = (i & 2) ? -2147483648.0f : 2147483648.0f; }
        run(c, w1, h1);
        c = base;
        c.s.gn_its = 16;
        for (int h = 0; h < c.F; ++h)
            for (int i = 0; i < c.n[h]; ++i) {
                Point& p = c.points[(size_t)h * c.max_points + i];
                const int side = i & 3;
                p.u = side == 0 ? 0.0f : side == 1 ? (float)(c.W - 1) : (float)(i % c.W);
                p.v = side == 2 ? 0.0f : side == 3 ? (float)(c.H - 1) : (float)(i % c.H);
            }
        run(c, w1, h1);
        c = base;
        c.s.gn_its = 16;
        for (Point& p : c.points) { p.idepth_min = 0.0f; p.idepth_max = 0.0f; }
        run(c, w1, h1);
        c = base;
        c.s.gn_its = 16;
        c.min_dist = 0.0f;
        run(c, w1, h1);
    }
    {   // a map of 3 x 3, and more seeds than cells
        Case c = base;
        run(c, 3, 3);
        c.n_active = 64;
        c.active_host.assign(64, c.newest == 0 ? 1 % c.F : 0);
        c.active.resize(3 * 64);
        for (int i = 0; i < 64; ++i) { c.active[3 * i] = (float)(i % 7); c.active[3 * i + 1] = (float)(i % 5); c.active[3 * i + 2] = 0.0f; }
        const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        for (int h = 0; h < c.F; ++h) { std::memcpy(&c.KRKi1[9 * h], I, sizeof(I)); c.Kt1[3 * h] = c.Kt1[3 * h + 1] = c.Kt1[3 * h + 2] = 0.0f; }
        run(c, 3, 3);
        run(c, w1, h1);
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    Reader r{std::fopen(argv[1], "rb")};
    if (!r.f) { std::perror(argv[1]); return 2; }
    const int ncases = r.i32();
    for (int k = 0; k < ncases; ++k) {
        Case c;
        c.H = r.i32(); c.W = r.i32(); c.F = r.i32(); c.max_points = r.i32(); c.newest = r.i32(); c.n_active = r.i32();
        r.get(&c.s, 1);
        c.huber = r.f32();
        r.get(c.K4, 4);
        c.min_dist = r.f32();
        if (!params_valid(c.s) || c.F < 1 || c.F > MAX_FRAMES || c.newest < 0 || c.newest >= c.F) { std::fprintf(stderr, "case %d: bad header\n", k); return 2; }
        c.n.resize(c.F); r.get(c.n.data(), c.n.size());
        c.points.resize((size_t)c.F * c.max_points); r.get(c.points.data(), c.points.size());
        c.colors.resize((size_t)c.F * c.H * c.W); r.get(c.colors.data(), c.colors.size());
        c.KRKi1.resize(9 * c.F); r.get(c.KRKi1.data(), c.KRKi1.size());
        c.Kt1.resize(3 * c.F); r.get(c.Kt1.data(), c.Kt1.size());
        c.active_host.resize(c.n_active); r.get(c.active_host.data(), c.active_host.size());
        c.active.resize(3 * (size_t)c.n_active); r.get(c.active.data(), c.active.size());
        c.flagged.resize(c.F); r.get(c.flagged.data(), c.flagged.size());
        c.pre.resize((size_t)c.F * c.F * PRE_WORDS); r.get(c.pre.data(), c.pre.size());
        run(c, c.W >> 1, c.H >> 1);
        if (c.F >= 3 && c.n_active > 0 && c.H * c.W <= 64 * 48) hostile(c);
    }
    std::fclose(r.f);
    std::printf("activate standalone: %d cases, %ld runs; zero cells %ld;", ncases, runs, zero_cells);
    const char* names[NUM_FATES] = {"NONE", "DELETED_UNTRACED", "DELETED_CANNOT", "KEPT_CANNOT", "DELETED_OUT_OF_MAP", "CHOSEN", "KEPT_TOO_CLOSE", "KEPT_WEAK",
                                    "DROPPED", "ACTIVATED"};
    for (int i = 0; i < NUM_FATES; ++i) std::printf(" %s %ld", names[i], hist[i]);
    std::printf("\n");
    return 0;
}
#endif
