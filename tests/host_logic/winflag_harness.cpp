// csrc/eds_winflag.hpp on the CPU: the rules of include/eds_hip_winflag.h over plain arrays, in the order of the device's steps
// (csrc/eds_winflag.hip and the history's part of csrc/eds_winedit.hip), bound by tests/winflag_harness.py, and — with
// -DWFL_STANDALONE — a program of its own that drives made-up windows with hostile values through them (for a sanitizer build; it is
// never loaded into python that way).  Built with g++ -ffp-contract=off.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../slam-eds_amd/csrc/eds_winedit.hpp"
#include "../../slam-eds_amd/csrc/eds_winflag.hpp"

using edswfl::Hist;

extern "C" {

void wfl_defaults(int n, int m, int32_t* num_good, float* max_rel, int32_t* last_target, int32_t* last_state, int32_t* is_new) {
    const Hist h = {num_good, max_rel, last_target, last_state, is_new};
    for (int p = 0; p < n; ++p) edswfl::default_point(h, p);
    for (int r = 0; r < m; ++r) is_new[r] = 1;
}

// the history of K activated points; mask[k] bit t: the fit left a residual towards frame t
void wfl_activated(int K, int F, const uint64_t* mask, int32_t* num_good, float* max_rel, int32_t* last_target, int32_t* last_state) {
    const Hist h = {num_good, max_rel, last_target, last_state, nullptr};
    for (int q = 0; q < K; ++q) edswfl::activated_point(h, q, F, (int)(mask[q] >> (F - 1) & 1u), F >= 2 ? (int)(mask[q] >> (F - 2) & 1u) : 0);
}

// the residuals with keep[r] == 0 leave while their points stay
void wfl_forget(int m, const int32_t* keep, const int32_t* point, const int32_t* target, int32_t* last_target) {
    for (int r = 0; r < m; ++r) if (!keep[r]) edswfl::forget_residual(last_target, point[r], target[r]);
}

void wfl_frames_down(int n, int frame, int32_t* last_target) {
    for (int i = 0; i < 2 * n; ++i) last_target[i] = edswfl::target_after(last_target[i], frame);
}

// makeKeyFrame's loop.  In: the tables and is_new (m).  Out: need (n), map new -> old (m + inserted, -1 for a new row), the new point
// / target / is_new columns; the point columns of the history change in place.  Returns the residuals inserted, or -1 beyond `capacity`
int wfl_insert_frame(int n, int m, int frame, int capacity, const int32_t* host, const int32_t* res_first, const int32_t* point, const int32_t* target,
                     const int32_t* is_new, int32_t* last_target, int32_t* last_state, int32_t* need, int32_t* map_r, int32_t* point_new, int32_t* target_new,
                     int32_t* is_new_new) {
    std::vector<int32_t> excl((size_t)n + 1), map_p((size_t)n + 1);
    for (int p = 0; p < n; ++p) need[p] = edswfl::needs_residual(res_first, target, host[p], p, frame);
    const int K = edswed::scan_serial(need, n, excl.data(), map_p.data());
    if (m + K > capacity) return -1;
    for (int i = 0; i < m + K; ++i) map_r[i] = -1;
    for (int r = 0; r < m; ++r) {
        const int i = edswfl::moved_row(excl.data(), point[r], r);
        map_r[i] = r; point_new[i] = point[r];
    }
    for (int i = 0; i < m + K; ++i) {                           // the gather: row map[i], zeros for a new row
        target_new[i] = map_r[i] < 0 ? 0 : target[map_r[i]];
        is_new_new[i] = map_r[i] < 0 ? 0 : is_new[map_r[i]];
    }
    const Hist h = {nullptr, nullptr, last_target, last_state, is_new_new};
    for (int p = 0; p < n; ++p) {
        if (!need[p]) continue;
        const int i = edswfl::new_row(res_first, excl.data(), p);
        point_new[i] = p; target_new[i] = frame; is_new_new[i] = 1;
        edswfl::shift_last(h, p, frame);
    }
    return K;
}

float wfl_rel_baseline(const float* pc, float u, float v, float idepth) { return edswfl::rel_baseline(pc, u, v, idepth); }

void wfl_apply_fixed(int n, int F, const float* pcs, const int32_t* host, const float* uv, const float* ids, const int32_t* res_first, const int32_t* target,
                     const int32_t* state, const int32_t* active, int32_t* num_good, float* max_rel, int32_t* last_target, int32_t* last_state, int32_t* is_new,
                     int clear_is_new, int32_t* counts) {
    const Hist h = {num_good, max_rel, last_target, last_state, is_new};
    counts[0] = counts[1] = counts[2] = 0;
    for (int p = 0; p < n; ++p)
        edswfl::apply_fixed_point(h, p, res_first, target, state, active, pcs, F, host[p], uv[2 * p], uv[2 * p + 1], ids[p], clear_is_new, counts);
}

// flagPointsForRemoval's decisions: phase one, then the Hessian for the candidates (what phase two re-linearizes in between changes
// nothing either reads).  prm4: the eds_wfl_params words.  Out: fate (n), candidate (n), counts (27)
void wfl_flag_points(int n, const int32_t* prm4, const int32_t* num_good, const int32_t* last_state, const int32_t* host, const float* ids,
                     const int32_t* res_first, const int32_t* target, const int32_t* state, const float* idepth_hessian, uint32_t frames_to_marg, int only_empty,
                     int32_t* fate, int32_t* candidate, int32_t* counts) {
    edswfl::Params prm;
    std::memcpy(&prm, prm4, sizeof(prm));
    const Hist h = {const_cast<int32_t*>(num_good), nullptr, nullptr, const_cast<int32_t*>(last_state), nullptr};
    for (int k = 0; k < 27; ++k) counts[k] = 0;
    for (int p = 0; p < n; ++p) {
        const int32_t f = edswfl::first_fate(prm, h, p, host[p], ids[p], res_first, target, state, frames_to_marg, only_empty);
        candidate[p] = f == edswfl::CANDIDATE;
        fate[p] = edswfl::finish_fate(prm, f, idepth_hessian[p]);
        ++counts[fate[p]];
        ++counts[3 + 3 * host[p] + fate[p]];
    }
}

}  // extern "C"

#ifdef WFL_STANDALONE
namespace {

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    int below(int k) { return (int)(next() % (uint32_t)k); }
    float unit() { return (float)(next() & 0xffffff) / (float)0x1000000; }
};

}  // namespace

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float hostile[] = {nan, inf, -inf, 0.0f, -0.0f, 1e38f, -1e-45f};
    long windows = 0, inserted = 0, forgotten = 0, passes = 0, refused = 0, flaggings = 0;
    for (int F = 2; F <= 8; ++F)
        for (int seed = 0; seed < 6; ++seed) {
            Rng g = {(uint64_t)(F * 977 + seed)};
            const int n = seed == 0 ? 0 : 1 + g.below(seed == 5 ? 3000 : 60);
            std::vector<int32_t> host((size_t)n), res_first((size_t)n + 1, 0), point, target;
            for (int p = 0; p < n; ++p) host[p] = (int)((int64_t)p * F / n);
            for (int p = 0; p < n; ++p) {
                for (int t = 0; t < F; ++t)
                    if (t != host[p] && g.below(3)) { point.push_back(p); target.push_back(t); }
                res_first[p + 1] = (int32_t)point.size();
            }
            int m = (int)point.size();
            std::vector<int32_t> ng((size_t)n), lt(2 * (size_t)n), ls(2 * (size_t)n), is_new((size_t)m), state((size_t)m), active((size_t)m);
            std::vector<float> mrb((size_t)n), uv(2 * (size_t)n), ids((size_t)n), pcs((size_t)F * F * 27);
            wfl_defaults(n, m, ng.data(), mrb.data(), lt.data(), ls.data(), is_new.data());
            for (int p = 0; p < n; ++p) {
                lt[2 * p] = g.below(F + 1) - 1; lt[2 * p + 1] = g.below(F + 1) - 1;
                ls[2 * p] = g.below(3); ls[2 * p + 1] = g.below(3);
                uv[2 * p] = 100.0f * g.unit(); uv[2 * p + 1] = 80.0f * g.unit();
                ids[p] = g.below(7) ? g.unit() : hostile[g.below(7)];
                mrb[p] = g.below(9) ? 0.1f * g.unit() : hostile[g.below(7)];
            }
            for (int r = 0; r < m; ++r) { state[r] = g.below(3); active[r] = g.below(2); is_new[r] = g.below(2) ? g.below(1 << 30) - (1 << 29) : 0; }
            for (float& v : pcs) v = g.below(11) ? 2.0f * g.unit() - 1.0f : hostile[g.below(7)];
            int32_t counts[3];
            wfl_apply_fixed(n, F, pcs.data(), host.data(), uv.data(), ids.data(), res_first.data(), target.data(), state.data(), active.data(), ng.data(), mrb.data(),
                            lt.data(), ls.data(), is_new.data(), seed & 1, counts);
            if (counts[0] + counts[1] + counts[2] != m) return 3;
            for (int p = 0; p < n; ++p) if (ng[p] < 0 || ng[p] > F) return 4;
            ++passes;
            // a third of the residuals leave, their points stay
            std::vector<int32_t> keep((size_t)m);
            for (int r = 0; r < m; ++r) { keep[r] = g.below(3) != 0; forgotten += !keep[r]; }
            wfl_forget(m, keep.data(), point.data(), target.data(), lt.data());
            for (int r = 0; r < m; ++r)
                if (!keep[r] && (lt[2 * point[r]] == target[r] || lt[2 * point[r] + 1] == target[r])) return 5;
            // every frame in turn gets its residuals, within and beyond the capacity
            for (int frame = 0; frame < F; ++frame) {
                std::vector<int32_t> need((size_t)n), map_r((size_t)m + n), pn((size_t)m + n), tn((size_t)m + n), nn((size_t)m + n);
                const std::vector<int32_t> lt0 = lt, ls0 = ls;
                const int rc = wfl_insert_frame(n, m, frame, m - 1, host.data(), res_first.data(), point.data(), target.data(), is_new.data(), lt.data(), ls.data(),
                                                need.data(), map_r.data(), pn.data(), tn.data(), nn.data());
                if (rc > 0 || lt != lt0 || ls != ls0) return 6;    // refused (or nothing to insert): nothing changed
                refused += rc < 0;
                const int K = wfl_insert_frame(n, m, frame, m + n, host.data(), res_first.data(), point.data(), target.data(), is_new.data(), lt.data(), ls.data(),
                                               need.data(), map_r.data(), pn.data(), tn.data(), nn.data());
                if (K < 0) return 7;
                m += K; inserted += K;
                point.assign(pn.begin(), pn.begin() + m); target.assign(tn.begin(), tn.begin() + m); is_new.assign(nn.begin(), nn.begin() + m);
                std::fill(res_first.begin(), res_first.end(), 0);
                for (int r = 0; r < m; ++r) { if (r && point[r] < point[r - 1]) return 8; ++res_first[point[r] + 1]; }
                for (int p = 0; p < n; ++p) res_first[p + 1] += res_first[p];
                for (int p = 0; p < n; ++p)
                    if (need[p] && (target[res_first[p + 1] - 1] != frame || lt[2 * p] != frame || ls[2 * p] != edswfl::ST_IN || !is_new[res_first[p + 1] - 1])) return 9;
            }
            for (int p = 0; p < n; ++p) if (res_first[p + 1] - res_first[p] != F - 1) return 10;   // every point now sees every other frame
            wfl_frames_down(n, F / 2, lt.data());
            for (int i = 0; i < 2 * n; ++i) if (lt[i] < -1 || lt[i] >= F) return 11;
            std::vector<uint64_t> mask((size_t)n);
            for (uint64_t& v : mask) v = g.next();
            wfl_activated(n, F, mask.data(), ng.data(), mrb.data(), lt.data(), ls.data());
            for (int p = 0; p < n; ++p) if ((lt[2 * p] == F - 1) != (ls[2 * p] == edswfl::ST_IN) || ng[p] || mrb[p] != 0.0f) return 12;
            // the flags, with hostile Hessians and every mask
            std::vector<int32_t> fate((size_t)n), cand((size_t)n);
            std::vector<float> hess((size_t)n);
            for (float& v : hess) v = g.below(5) ? 100.0f * g.unit() : hostile[g.below(7)];
            state.assign((size_t)m, 0);                         // the tables grew with the inserts
            for (int r = 0; r < m; ++r) state[r] = g.below(3);
            const edswfl::Params prm = edswfl::params_default();
            int32_t prm4[4], c27[27];
            std::memcpy(prm4, &prm, sizeof(prm));
            for (uint32_t mask = 0; mask < (1u << F); mask += 1 + (uint32_t)g.below(5))
                for (int only_empty = 0; only_empty < 2; ++only_empty) {
                    wfl_flag_points(n, prm4, ng.data(), ls.data(), host.data(), ids.data(), res_first.data(), target.data(), state.data(), hess.data(), mask, only_empty,
                                    fate.data(), cand.data(), c27);
                    if (c27[0] + c27[1] + c27[2] != n) return 13;
                    for (int p = 0; p < n; ++p) if (fate[p] < 0 || fate[p] > 2 || (only_empty && fate[p] == 1)) return 14;
                    ++flaggings;
                }
            ++windows;
        }
    std::printf("winflag standalone: %ld windows; %ld passes, %ld residuals inserted, %ld forgotten, %ld refused, %ld flaggings\n", windows, passes, inserted, forgotten,
                refused, flaggings);
    return 0;
}
#endif
