// Activation of DSO's immature points (include/eds_hip_activate.h): what the device kernels (eds_activate.hip) and the host share — the
// projection into the coarse distance map, one round of growDistBFS in the two forms the kernels run (from every cell after seeding,
// from one seed's frontier in the candidate loop), the candidate rule, one tap of ImmaturePoint::linearizeResidual and the Gauss-Newton
// loop around it — and serial evaluators (make_map_serial, select_body with one thread, fit_serial) that the CPU tests compare with the
// numpy oracle.  fp32 in the reference's order; every translation unit that includes this is built without contraction into FMAs.
// Plain C++ outside hipcc.  The sample is edsimm::interp33 on the eds_imm's own {colour, gradient} planes; the long projectPoint
// overload is restated here per tap (edswin::geo restates it for the centre pixel only and with its Jacobians).
//
// THE MAP.  One byte per cell: 0 ... 39, and FAR = 255 for the reference's 1000.  A round k of growDistBFS sets cells to k that were
// above k and takes its frontier from round k - 1, so after seeding from an all-FAR map "value == k - 1" IS "set in round k - 1" and a
// round is one pass over the cells (grow_pull).  In the candidate loop the map already holds values, so a frontier cell is told by a
// tag: mark[cell] = serial * 64 + round, serial counting the chosen points of this selection from 1 (grow_takes).
#pragma once
#include "eds_immature.hpp"

namespace edsact {

using edsimm::finite_f;
using edsimm::Frame;
using edsimm::Grad;
using edsimm::Point;

constexpr int MAX_FRAMES = 64;                       // a residual set is one wavefront's ballot
constexpr int PATTERN = 8;
constexpr int ROUNDS = 39;                           // growDistBFS: k = 1 ... 39
constexpr int FAR = 255;                             // the byte that stands for 1000
constexpr int PRE_WORDS = 14;                        // PRE_RTll (9), PRE_tTll (3), PRE_aff_mode (2)
enum { ST_IN = 0, ST_OOB = 1, ST_OUTLIER = 2 };      // ResState

enum Fate : int32_t {
    NONE = 0, DELETED_UNTRACED = 1, DELETED_CANNOT = 2, KEPT_CANNOT = 3, DELETED_OUT_OF_MAP = 4, CHOSEN = 5, KEPT_TOO_CLOSE = 6, KEPT_WEAK = 7,
    DROPPED = 8, ACTIVATED = 9
};
constexpr int NUM_FATES = 10;

// eds_act_params, member for member
struct Params {
    float min_idepth_h_act;
    int32_t gn_its;
    float min_trace_quality, max_trace_pixel_interval;
    int32_t min_obs;
    float scale_idepth;
};

struct Calib { float fx, fy, cx, cy, fxli, fyli, wM3G, hM3G; int32_t W, H, w1, h1; };

EDS_HD Params params_default() { Params p = {100.0f, 3, 3.0f, 8.0f, 1, 1.0f}; return p; }
EDS_HD bool params_valid(const Params& p) {
    return finite_f(p.min_idepth_h_act) && finite_f(p.min_trace_quality) && finite_f(p.max_trace_pixel_interval) && finite_f(p.scale_idepth) &&
           p.scale_idepth > 0.0f && p.gn_its >= 0 && p.gn_its <= 16 && p.min_obs >= 0 && p.min_obs <= MAX_FRAMES;
}
EDS_HD Calib make_calib(int H, int W, float fx, float fy, float cx, float cy) {
    Calib c;
    c.fx = fx; c.fy = fy; c.cx = cx; c.cy = cy; c.fxli = 1.0f / fx; c.fyli = 1.0f / fy;
    c.wM3G = (float)(W - 3); c.hM3G = (float)(H - 3); c.W = W; c.H = H; c.w1 = W >> 1; c.h1 = H >> 1;
    return c;
}

EDS_HD float map_value(uint8_t b) { return b == FAR ? 1000.0f : (float)b; }
EDS_HD bool on_ring(int x, int y, int w1, int h1) { return x == 0 || y == 0 || x == w1 - 1 || y == h1 - 1; }

// ptp = KRKi (u, v, 1) + Kt idepth, every row summed left to right; the cell (int)(ptp0 / ptp2 + 0.5f), (int)(ptp1 / ptp2 + 0.5f) when it
// lies inside the map.  A quotient that is not finite or beyond +-2^20 is outside: the conversion is never reached.
EDS_HD bool map_cell(const float* K, const float* Kt, float u, float v, float idepth, int w1, int h1, int* u1, int* v1, float* ptp0) {
    const float p0 = ((K[0] * u + K[1] * v) + K[2] * 1.0f) + Kt[0] * idepth;
    const float p1 = ((K[3] * u + K[4] * v) + K[5] * 1.0f) + Kt[1] * idepth;
    const float p2 = ((K[6] * u + K[7] * v) + K[8] * 1.0f) + Kt[2] * idepth;
    const float qu = p0 / p2, qv = p1 / p2;
    if (!(fabsf(qu) <= 1048576.0f && fabsf(qv) <= 1048576.0f)) return false;
    const int a = (int)(qu + 0.5f), b = (int)(qv + 0.5f);
    if (!(a > 0 && b > 0 && a < w1 && b < h1)) return false;
    *u1 = a; *v1 = b; *ptp0 = p0;
    return true;
}

// the neighbourhood of round k: the first four offsets always, all eight when k is odd
EDS_HD int nb_count(int k) { return (k & 1) ? 8 : 4; }
EDS_HD int nb_x(int i) { const int t[8] = {1, -1, 0, 0, 1, -1, -1, 1}; return t[i]; }
EDS_HD int nb_y(int i) { const int t[8] = {0, 0, 1, -1, 1, 1, -1, -1}; return t[i]; }

// round k after seeding: cell (x, y) is set to k when it is above k and a neighbour that is not on the ring holds k - 1
EDS_HD bool grow_pull(const uint8_t* map, int w1, int h1, int k, int x, int y) {
    if ((int)map[x + y * w1] <= k) return false;
    const int nn = nb_count(k);
    for (int i = 0; i < nn; ++i) {
        const int nx = x + nb_x(i), ny = y + nb_y(i);
        if (nx < 0 || ny < 0 || nx >= w1 || ny >= h1 || on_ring(nx, ny, w1, h1)) continue;
        if ((int)map[nx + ny * w1] == k - 1) return true;
    }
    return false;
}

// round k of one seed's grow: ... when it is above k and a neighbour that is not on the ring was taken in round k - 1 OF THIS GROW
EDS_HD bool grow_takes(const uint8_t* map, const uint32_t* mark, int w1, int h1, int k, int x, int y, uint32_t prev_tag) {
    if ((int)map[x + y * w1] <= k) return false;
    const int nn = nb_count(k);
    for (int i = 0; i < nn; ++i) {
        const int nx = x + nb_x(i), ny = y + nb_y(i);
        if (nx < 0 || ny < 0 || nx >= w1 || ny >= h1 || on_ring(nx, ny, w1, h1)) continue;
        if (mark[nx + ny * w1] == prev_tag) return true;
    }
    return false;
}

// canActivate of the stated loop
EDS_HD bool can_activate(const Point& p, const Params& s) {
    const bool st = p.status == edsimm::GOOD || p.status == edsimm::SKIPPED || p.status == edsimm::BADCONDITION || p.status == edsimm::OOB;
    return st && p.last_interval < s.max_trace_pixel_interval && p.quality > s.min_trace_quality && (p.idepth_max + p.idepth_min) > 0;
}

// rows a and b of the candidate rule; NONE: go on to the map
EDS_HD int fate_before_map(const Point& p, const Params& s, bool host_flagged) {
    if (!finite_f(p.idepth_max) || p.status == edsimm::OUTLIER) return DELETED_UNTRACED;
    if (!can_activate(p, s)) return (host_flagged || p.status == edsimm::OOB) ? DELETED_CANNOT : KEPT_CANNOT;
    return NONE;
}

struct SelectIn {
    const Point* points; int max_points; const int32_t* n; int newest, n_hosts;
    const float* KRKi1; const float* Kt1; const uint8_t* flagged; float min_act_dist;
    Params prm; int w1, h1;
    uint8_t* map; uint32_t* mark; int32_t* fate; int32_t* counts;
};

// The candidate loop, written once over a thread index, a thread count and a barrier: one workgroup runs it on the device, the host
// with one thread.  sync.barrier() orders the map's reads and writes; sync.any(b) is a barrier that returns whether any thread passed
// true.  Every thread takes every decision from the same values, so control flow is uniform.
template <class Sync>
EDS_HD void select_body(const SelectIn& in, int tid, int nt, Sync& sync) {
    int cnt[NUM_FATES];
    for (int i = 0; i < NUM_FATES; ++i) cnt[i] = 0;
    const int w1 = in.w1, h1 = in.h1;
    for (int c = tid; c < w1 * h1; c += nt) in.mark[c] = 0u;
    sync.barrier();
    uint32_t serial = 0;
    for (int h = 0; h < in.n_hosts; ++h) {
        int32_t* fate = in.fate + (size_t)h * in.max_points;
        const int n = in.n[h];
        if (h == in.newest) {
            for (int i = tid; i < n; i += nt) fate[i] = NONE;
            continue;
        }
        const Point* pts = in.points + (size_t)h * in.max_points;
        const float* K = in.KRKi1 + 9 * h;
        const float* Kt = in.Kt1 + 3 * h;
        for (int i = 0; i < n; ++i) {
            const Point& p = pts[i];
            int f = NONE;
            int u1 = 0, v1 = 0;
            if (p.alive) {
                f = fate_before_map(p, in.prm, in.flagged[h] != 0);
                if (f == NONE) {
                    float ptp0 = 0.0f;
                    if (!map_cell(K, Kt, p.u, p.v, 0.5f * (p.idepth_max + p.idepth_min), w1, h1, &u1, &v1, &ptp0)) {
                        f = DELETED_OUT_OF_MAP;
                    } else {
                        const float dist = map_value(in.map[u1 + w1 * v1]) + (ptp0 - floorf(ptp0));
                        f = dist >= in.min_act_dist * p.type ? CHOSEN : KEPT_TOO_CLOSE;
                    }
                }
                ++cnt[f];
            }
            if (tid == 0) fate[i] = f;
            if (f != CHOSEN) continue;
            // addIntoDistFinal(u1, v1)
            ++serial;
            sync.barrier();                                      // every thread has read the cell
            if (tid == 0) { in.map[u1 + w1 * v1] = 0; in.mark[u1 + w1 * v1] = serial << 6; }
            sync.barrier();
            for (int k = 1; k <= ROUNDS; ++k) {
                const int x0 = u1 - k < 0 ? 0 : u1 - k, x1 = u1 + k > w1 - 1 ? w1 - 1 : u1 + k;
                const int y0 = v1 - k < 0 ? 0 : v1 - k, y1 = v1 + k > h1 - 1 ? h1 - 1 : v1 + k;
                const int wx = x1 - x0 + 1, total = wx * (y1 - y0 + 1);
                const uint32_t prev = (serial << 6) | (uint32_t)(k - 1), tag = (serial << 6) | (uint32_t)k;
                bool took = false;
                for (int c = tid; c < total; c += nt) {
                    const int x = x0 + c % wx, y = y0 + c / wx;
                    if (grow_takes(in.map, in.mark, w1, h1, k, x, y, prev)) {
                        in.map[x + y * w1] = (uint8_t)k;
                        in.mark[x + y * w1] = tag;
                        took = true;
                    }
                }
                if (!sync.any(took)) break;
            }
        }
    }
    if (tid == 0) for (int i = 0; i < NUM_FATES; ++i) in.counts[i] = cnt[i];
}

struct SerialSync {
    void barrier() {}
    bool any(bool b) { return b; }
};

// ---- one tap of ImmaturePoint::linearizeResidual (ImmaturePoint.cpp:550-581) -------------------------------------------------------------
// fail: 0 none, 1 projectPoint (ResidualProjections.h:60-86) refused, 2 a non-finite colour.  e, h, b: the tap's addends to energyLeft,
// Hdd and bd.  pre: PRE_RTll row-major, PRE_tTll, PRE_aff_mode.
struct TapOut { int32_t fail; float e, h, b; };

EDS_HD TapOut tap(const Calib& K, float scale_idepth, float huber, const float* pre, const Frame& f, const Point& p, float idepth, int idx) {
    TapOut o;
    o.fail = 1; o.e = o.h = o.b = 0.0f;
    const float* R = pre;
    const float* t = pre + 9;
    const float k0 = ((p.u + (float)edsimm::pat_x(idx)) - K.cx) * K.fxli, k1 = ((p.v + (float)edsimm::pat_y(idx)) - K.cy) * K.fyli;
    const float p0 = ((R[0] * k0 + R[1] * k1) + R[2] * 1.0f) + t[0] * idepth;
    const float p1 = ((R[3] * k0 + R[4] * k1) + R[5] * 1.0f) + t[1] * idepth;
    const float p2 = ((R[6] * k0 + R[7] * k1) + R[8] * 1.0f) + t[2] * idepth;
    const float drescale = 1.0f / p2;
    if (!(drescale > 0)) return o;
    const float u = p0 * drescale, v = p1 * drescale;
    const float Ku = u * K.fx + K.cx, Kv = v * K.fy + K.cy;
    if (!(Ku > 1.1f && Kv > 1.1f && Ku < K.wM3G && Kv < K.hM3G)) return o;
    float hit[3];
    edsimm::interp33(f, K.W, K.H, Ku, Kv, hit);
    if (!finite_f(hit[0])) { o.fail = 2; return o; }
    o.fail = 0;
    const float residual = hit[0] - (pre[12] * p.color[idx] + pre[13]);
    float hw = fabsf(residual) < huber ? 1 : huber / fabsf(residual);
    const float w = p.weights[idx];
    o.e = w * w * hw * residual * residual * (2 - hw);
    const float dxInterp = hit[1] * K.fx, dyInterp = hit[2] * K.fy;
    const float d = (dxInterp * drescale * (t[0] - t[2] * u) + dyInterp * drescale * (t[1] - t[2] * v)) * scale_idepth;
    hw *= w * w;
    o.h = (hw * d) * d;
    o.b = (hw * residual) * d;
    return o;
}

// the target frame of residual r of a point hosted by `host`: the frames 0 ... n_hosts - 1 except the host, in that order
EDS_HD int res_target(int host, int r) { return r < host ? r : r + 1; }

// what linearizeResidual leaves after its last tap (:584-595)
EDS_HD void verdict(float energy, float energyTH, float slack, int32_t* new_state, float* new_energy) {
    if (energy > energyTH * slack) { energy = energyTH * slack; *new_state = ST_OUTLIER; }
    else *new_state = ST_IN;
    *new_energy = energy;
}

struct Sums { float E, Hdd, bd; };
struct Fit { int32_t fate; float idepth, E, Hdd, bd; };

// The stated optimizeImmaturePoint loop over an evaluator: ev.eval(idepth, slack) runs linearizeResidual over the residuals in order,
// ev.apply() is state = new_state, energy = new_energy for every residual, ev.count_in() the residuals whose state is IN.
template <class Ev>
EDS_HD Fit fit_loop(Ev& ev, const Params& s, const Point& p) {
    float idepth = (p.idepth_max + p.idepth_min) * 0.5f;
    Sums c = ev.eval(idepth, 1000.0f);
    ev.apply();
    Fit o;
    o.fate = KEPT_WEAK;
    if (finite_f(c.E) && !(c.Hdd < s.min_idepth_h_act)) {
        o.fate = NONE;
        float lambda = 0.1f;
        for (int it = 0; it < s.gn_its; ++it) {
            float H = c.Hdd;
            H *= 1 + lambda;
            const float step = (float)((1.0 / (double)H) * (double)c.bd);
            const float nid = idepth - step;
            const Sums n = ev.eval(nid, 1.0f);
            if (!finite_f(c.E) || n.Hdd < s.min_idepth_h_act) { o.fate = KEPT_WEAK; break; }
            if (n.E < c.E) { idepth = nid; c = n; ev.apply(); lambda *= 0.5f; }
            else lambda *= 5;
            if ((double)fabsf(step) < 0.0001 * (double)idepth) break;
        }
        if (o.fate == NONE) o.fate = (!finite_f(idepth) || ev.count_in() < s.min_obs) ? DROPPED : ACTIVATED;
    }
    o.idepth = idepth; o.E = c.E; o.Hdd = c.Hdd; o.bd = c.bd;
    return o;
}

// a fitted point leaves the immature set, as does everything the candidate rule deleted
EDS_HD bool leaves(int fate, int status) {
    return fate == ACTIVATED || fate == DROPPED || (fate == KEPT_WEAK && status == edsimm::OOB) || fate == DELETED_UNTRACED ||
           fate == DELETED_CANNOT || fate == DELETED_OUT_OF_MAP;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the serial side ---------------------------------------------------------------------------------------------------------------------
// makeDistanceMap in the round form: every cell FAR, the seeds 0, then the 39 rounds
inline void make_map_serial(uint8_t* map, int w1, int h1, int newest, const float* KRKi1, const float* Kt1, int n_active, const int32_t* active_host,
                            const float* active) {
    for (int i = 0; i < w1 * h1; ++i) map[i] = (uint8_t)FAR;
    for (int i = 0; i < n_active; ++i) {
        const int h = active_host[i];
        if (h == newest) continue;
        int u1, v1;
        float p0;
        if (map_cell(KRKi1 + 9 * h, Kt1 + 3 * h, active[3 * i], active[3 * i + 1], active[3 * i + 2], w1, h1, &u1, &v1, &p0)) map[u1 + w1 * v1] = 0;
    }
    for (int k = 1; k <= ROUNDS; ++k)
        for (int y = 0; y < h1; ++y)
            for (int x = 0; x < w1; ++x)
                if (grow_pull(map, w1, h1, k, x, y)) map[x + y * w1] = (uint8_t)k;
}

struct SerialEval {
    const Calib* K; float scale_idepth, huber; const float* pre; const float* c; const Grad* g; const Point* p; int host, n_hosts;
    int32_t state[MAX_FRAMES], new_state[MAX_FRAMES];
    float energy[MAX_FRAMES], new_energy[MAX_FRAMES];
    Sums eval(float idepth, float slack) {
        Sums a = {0.0f, 0.0f, 0.0f};
        const size_t px = (size_t)K->W * K->H;
        for (int r = 0; r < n_hosts - 1; ++r) {
            float ret = energy[r];
            if (state[r] == ST_OOB) { new_state[r] = ST_OOB; }
            else {
                const int t = res_target(host, r);
                const Frame f = {c + px * t, g + px * t};
                float e = 0;
                int k = 0;
                for (; k < PATTERN; ++k) {
                    const TapOut o = tap(*K, scale_idepth, huber, pre + (size_t)(host * n_hosts + t) * PRE_WORDS, f, *p, idepth, k);
                    if (o.fail) break;
                    e += o.e; a.Hdd += o.h; a.bd += o.b;
                }
                if (k < PATTERN) new_state[r] = ST_OOB;
                else { verdict(e, p->energyTH, slack, &new_state[r], &new_energy[r]); ret = new_energy[r]; }
            }
            a.E = (float)((double)a.E + (double)ret);
        }
        return a;
    }
    void apply() { for (int r = 0; r < n_hosts - 1; ++r) { state[r] = new_state[r]; energy[r] = new_energy[r]; } }
    int count_in() const { int n = 0; for (int r = 0; r < n_hosts - 1; ++r) n += state[r] == ST_IN; return n; }
};

// one CHOSEN point's fit; res_state / res_energy: n_hosts words, the host's own column -1 / 0
inline Fit fit_serial(const Calib& K, const Params& s, float huber, const float* pre, const float* c, const Grad* g, const Point& p, int host, int n_hosts,
                      int32_t* res_state, float* res_energy) {
    SerialEval ev;
    ev.K = &K; ev.scale_idepth = s.scale_idepth; ev.huber = huber; ev.pre = pre; ev.c = c; ev.g = g; ev.p = &p; ev.host = host; ev.n_hosts = n_hosts;
    for (int r = 0; r < MAX_FRAMES; ++r) { ev.state[r] = ev.new_state[r] = ST_IN; ev.energy[r] = ev.new_energy[r] = 0.0f; }
    const Fit o = fit_loop(ev, s, p);
    for (int t = 0; t < n_hosts; ++t) { res_state[t] = -1; res_energy[t] = 0.0f; }
    for (int r = 0; r < n_hosts - 1; ++r) { res_state[res_target(host, r)] = ev.state[r]; res_energy[res_target(host, r)] = ev.energy[r]; }
    return o;
}
#endif

}  // namespace edsact
