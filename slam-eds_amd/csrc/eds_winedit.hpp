// The window's tables edited in place of a read-back (include/eds_hip_winedit.h): what the device kernels (eds_winedit.hip) and the
// host share — which rows survive, the exclusive prefix sum that numbers them (its serial form; the device forms the same integers in
// three passes), the move of one word or one 16-byte piece of a surviving row, the renumbering of a residual's point, a point's new
// first residual, and the window's host copies after an edit.  Integers and copies only: nothing is rounded, so host and device agree
// by construction as long as both move the same rows.  Plain C++ outside hipcc.
//
// THE ORDER.  Every edit is stable: row i of the new table is row map[i] of the old one with map increasing.  The reference's
// swap-with-back is not restated (include/eds_hip_winedit.h says why).
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "eds_dso_common.hpp"

namespace edswed {

constexpr int ST_IN = 0;                                        // ResState::IN (Residuals.h:47)
constexpr int MAX_FRAMES = 8;
constexpr int WIDE_WORDS = 74;                                  // one RawResidualJacobian: J and ef_J
constexpr int WIDE_PIECES = 19;                                 // 18 pieces of 16 bytes and one of 8: 296 bytes
constexpr int MAX_COLS = 24;
constexpr int SCAN_TB = 256, SCAN_ITEMS = 4, SCAN_TILE = SCAN_TB * SCAN_ITEMS;   // one workgroup of the device's scan numbers 1 024 rows

// one column of a table: `words` 32-bit words a row, `first` words of the columns before it
struct Col { const char* src; char* dst; int32_t words, first; };
struct Cols { int32_t count, words; Col c[MAX_COLS]; };

inline void cols_clear(Cols& t) { t.count = 0; t.words = 0; }
inline void cols_add(Cols& t, const void* src, void* dst, int words) {
    Col& c = t.c[t.count++];
    c.src = static_cast<const char*>(src); c.dst = static_cast<char*>(dst); c.words = words; c.first = t.words;
    t.words += words;
}

// ---- which rows stay ---------------------------------------------------------------------------------------------------------------------
// eds_wed_remove_residuals: select given, the residuals it marks go; select == NULL, every residual whose state is not IN goes
EDS_HD int32_t keep_residual(const int32_t* select, const int32_t* state, int r) { return select ? select[r] == 0 : state[r] == ST_IN; }
// eds_wed_remove_points: a flagged point goes, and a residual goes with its point
EDS_HD int32_t keep_point(const int32_t* flag, int p) { return flag[p] == 0; }
EDS_HD int32_t keep_residual_of(const int32_t* keep_point_, const int32_t* res_point, int r) { return keep_point_[res_point[r]]; }

// excl[i] = the kept rows before row i, excl[n] = all of them; map[excl[i]] = i for every kept row.  Returns excl[n].
inline int scan_serial(const int32_t* keep, int n, int32_t* excl, int32_t* map) {
    int run = 0;
    for (int i = 0; i < n; ++i) {
        excl[i] = run;
        if (keep[i]) map[run++] = i;
    }
    excl[n] = run;
    return run;
}

// ---- moving the rows -----------------------------------------------------------------------------------------------------------------------
// both sides copy through the compiler's memcpy with a constant size: no pointer is read through another type
template <int BYTES, int ALIGN> EDS_HD void copy_bytes(char* dst, const char* src) {
    __builtin_memcpy(__builtin_assume_aligned(dst, ALIGN), __builtin_assume_aligned(src, ALIGN), BYTES);
}
template <int BYTES, int ALIGN> EDS_HD void zero_bytes(char* dst) { __builtin_memset(__builtin_assume_aligned(dst, ALIGN), 0, BYTES); }
// map[i] < 0: row i is new (eds_wed_insert_activated): every word of it starts as 0

// word g of the narrow columns: new row g / t.words, word g % t.words of the row, counted over the columns one after the other
EDS_HD void move_word(const Cols& t, const int32_t* map, int64_t g) {
    const int64_t i = g / t.words;
    const int w = (int)(g % t.words);
    int k = 0;
    while (w >= t.c[k].first + t.c[k].words) ++k;
    const Col& c = t.c[k];
    const int64_t off = w - c.first;
    if (map[i] < 0) zero_bytes<4, 4>(c.dst + 4 * ((int64_t)i * c.words + off));
    else copy_bytes<4, 4>(c.dst + 4 * ((int64_t)i * c.words + off), c.src + 4 * ((int64_t)map[i] * c.words + off));
}

// piece g of a 74-word column: new row g / 19, piece g % 19.  A row starts at a multiple of 296 bytes, so a piece is aligned to 8.
EDS_HD void move_wide(const char* src, char* dst, const int32_t* map, int64_t g) {
    const int64_t i = g / WIDE_PIECES;
    const int c = (int)(g % WIDE_PIECES);
    char* d = dst + 4 * (i * WIDE_WORDS) + 16 * c;
    if (map[i] < 0) {
        if (c < WIDE_PIECES - 1) zero_bytes<16, 8>(d);
        else zero_bytes<8, 8>(d);
        return;
    }
    const char* s = src + 4 * ((int64_t)map[i] * WIDE_WORDS) + 16 * c;
    if (c < WIDE_PIECES - 1) copy_bytes<16, 8>(d, s);
    else copy_bytes<8, 8>(d, s);
}

// the point of new residual i: its old point's new index (new_point == NULL: the points did not move)
EDS_HD int32_t moved_res_point(const int32_t* res_point, const int32_t* map_r, const int32_t* new_point, int i) {
    const int32_t p = res_point[map_r[i]];
    return new_point ? new_point[p] : p;
}
// the first residual of new point q (q = n_new: the end of the table): the kept residuals before its old first one
EDS_HD int32_t moved_res_first(const int32_t* res_first, const int32_t* map_p, const int32_t* excl_r, int q, int n_new, int m_new) {
    if (q >= n_new) return m_new;
    return excl_r[res_first[map_p ? map_p[q] : q]];
}

// ---- the window's host copies ----------------------------------------------------------------------------------------------------------------
struct Mirrors {
    std::vector<int32_t> host_of, point, target;               // per point; per residual
    int n = 0, m = 0, max_host = -1, max_target = -1;
};
// keep_p == NULL: the points stay.  The same rule as the tables': stable, points renumbered.
inline void edit_mirrors(Mirrors& w, const int32_t* keep_p, const int32_t* keep_r) {
    std::vector<int32_t> new_point((size_t)w.n);
    int n2 = 0;
    for (int p = 0; p < w.n; ++p) {
        new_point[p] = n2;
        if (!keep_p || keep_p[p]) w.host_of[n2++] = w.host_of[p];
    }
    int m2 = 0;
    for (int r = 0; r < w.m; ++r) {
        if (!keep_r[r]) continue;
        w.point[m2] = new_point[w.point[r]];
        w.target[m2++] = w.target[r];
    }
    w.n = n2; w.m = m2;
    w.host_of.resize((size_t)n2); w.point.resize((size_t)m2); w.target.resize((size_t)m2);
    w.max_host = w.max_target = -1;
    for (int p = 0; p < n2; ++p) if (w.host_of[p] > w.max_host) w.max_host = w.host_of[p];
    for (int r = 0; r < m2; ++r) if (w.target[r] > w.max_target) w.max_target = w.target[r];
}
inline void per_host_counts(const std::vector<int32_t>& host_of, int32_t* per_host) {
    for (int f = 0; f < MAX_FRAMES; ++f) per_host[f] = 0;
    for (int32_t h : host_of) if (h >= 0 && h < MAX_FRAMES) ++per_host[h];
}

// ---- activated points enter (eds_wed_insert_activated) ------------------------------------------------------------------------------------
// The candidates are the immature points in (host, index) order, candidate c = host * mp + index; the grid is (candidate, target),
// g = c * F + t.  A candidate enters when its fate is ACTIVATED; a grid cell becomes a residual when its candidate enters and the
// fit's residual state towards t is IN.  excl_c / excl_g are the exclusive sums of those two flag arrays.  Per host the window's own
// points come first, in order, then the host's activated points in index order; a new point's residuals in ascending target.
constexpr int ST_OUTLIER = 2, FATE_ACTIVATED = 9;
struct ImmCounts { int32_t n[MAX_FRAMES]; };                    // immature points per host
EDS_HD int32_t ins_keep_candidate(const ImmCounts& nn, const int32_t* fate, int mp, int c) {
    return c % mp < nn.n[c / mp] && fate[c] == FATE_ACTIVATED;
}
EDS_HD int32_t ins_keep_cell(const ImmCounts& nn, const int32_t* fate, const int32_t* res_state, int F, int mp, int stride, int64_t g) {
    const int c = (int)(g / F), t = (int)(g % F);
    return ins_keep_candidate(nn, fate, mp, c) && res_state[(int64_t)c * stride + t] == ST_IN;
}
struct Ins {
    int F, mp;
    const int32_t *first, *res_first;                           // the window's hosts' runs [9] and res_first [n + 1] BEFORE the insert
    const int32_t *excl_c, *excl_g;
};
EDS_HD int ins_old_point(const Ins& s, int p, int host) { return p + s.excl_c[host * s.mp]; }
EDS_HD int ins_new_point(const Ins& s, int c) { return s.first[c / s.mp + 1] + s.excl_c[c]; }
EDS_HD int ins_old_res(const Ins& s, int r, int host) { return r + s.excl_g[(int64_t)host * s.mp * s.F]; }
EDS_HD int ins_new_res(const Ins& s, int64_t g) { return s.res_first[s.first[(int)(g / s.F) / s.mp + 1]] + s.excl_g[g]; }

// ---- a frame leaves: the tables ----------------------------------------------------------------------------------------------------------------
// every residual towards the frame goes (FullSystem drops them before marginalizeFrame); hosts and targets above it go down by one
EDS_HD int32_t keep_residual_not_towards(const int32_t* res_target, int frame, int r) { return res_target[r] != frame; }
EDS_HD int32_t frame_after(int32_t f, int frame) { return f > frame ? f - 1 : f; }

// ---- a frame leaves: EnergyFunctional::marginalizeFrame's arithmetic (EnergyFunctional.cpp:516-576), fp64 -----------------------------------
// N = 4 + 8 F, nd = N - 8.  In the order of the reference's lines, every step by the thread that owns its entry:
//  1. the frame's block to the end (:516-536): P(i) = i below io = 4 + 8 frame, i + 8 from io to nd - 1, io + (i - nd) from nd on;
//     H_ij <- HM[P(i)][P(j)], b_i <- bM[P(i)].  The last frame takes no branch in the reference; P is then the identity.
//  2. H_(nd+k)(nd+k) += prior[k]; b_(nd+k) += prior[k] * delta_prior[k]: one product and one add (:540-541).
//  3. S_i = sqrt(|H_ii| + 10), SI_i = 1 / S_i (:548-549).
//  4. H_ij <- (SI_i * H_ij) * SI_j, b_i <- SI_i * b_i (:556-557).
//  5. hpi = the inverse of the trailing 8 x 8 (:560-563; 0.5f * (hpi + hpi) is hpi exactly, before and after).  Eigen's inverse cannot
//     be pinned, so the inverse is STATED, as the solve's LDLT is: an LU with partial pivoting by ONE thread.  For k = 0 .. 7 the pivot
//     is the row r >= k of largest |a_rk|, the lowest r on a tie; rows k and r change places whole; l_rk = a_rk / a_kk and
//     a_rc <- a_rc - l_rk * a_kc for r, c > k.  Then, for each column e of the identity, y_i = rhs_i - (sum over j < i of l_ij y_j) and
//     x_i = (y_i - (sum over j > i of u_ij x_j)) / u_ii, each sum from 0.0 in ascending j and then ONE subtraction; hpi_ie = x_i.
//     A pivot that is exactly 0, or an entry of hpi that is not finite, sets the flag: nothing is written.
//  6. bli_ik = sum over j = 0 .. 7 of B_ji hpi_jk from 0.0 in ascending j, B the bottom-left 8 x nd block (:566).
//  7. T_ij = A_ij - (sum over k of bli_ik B_kj), the sum from 0.0 in ascending k and then one subtraction; b_i likewise with the tail of
//     b (:567-568).
//  8. H_ij <- (S_i * T_ij) * S_j, b_i <- S_i * b_i (:571-572).
//  9. HM'_ij = 0.5 * (H_ij + H_ji), bM'_i = b_i (:575-576).  An entry that is not finite sets the flag.
constexpr int MAX_N = 4 + 8 * MAX_FRAMES;                       // 68
struct MargMem {
    double H[MAX_N * MAX_N], b[MAX_N], S[MAX_N], SI[MAX_N], bli[(MAX_N - 8) * 8], hpi[64], lu[64];
    int32_t bad;
};
struct MargIo {
    int N, frame;
    const double *HM, *bM, *prior, *delta_prior;                // N x N, N, 8, 8
    double *HM_out, *bM_out;                                    // (N - 8) x (N - 8), N - 8; may be HM, bM: everything is read before anything is written
    int32_t* flag;                                              // set to 1 where the header says EDS_ERR_NOT_USABLE
};
EDS_HD bool finite_d(double v) { return v - v == 0.0; }
EDS_HD int marg_perm(int i, int io, int nd) { return i < io ? i : i < nd ? i + 8 : io + (i - nd); }

// step 5, by one thread: a[64] row-major in (the LU overwrites it), hpi[64] out; false for a zero pivot or a result that is not finite
EDS_HD bool inverse8(double* a, double* hpi) {
    int perm[8];
    for (int i = 0; i < 8; ++i) perm[i] = i;
    for (int k = 0; k < 8; ++k) {
        int p = k;
        double best = a[k * 8 + k] < 0 ? -a[k * 8 + k] : a[k * 8 + k];
        for (int r = k + 1; r < 8; ++r) {
            const double v = a[r * 8 + k] < 0 ? -a[r * 8 + k] : a[r * 8 + k];
            if (v > best) { best = v; p = r; }
        }
        if (!(a[p * 8 + k] != 0.0)) return false;                // a zero pivot; a NaN column fails here as well
        if (p != k) {
            for (int c = 0; c < 8; ++c) { const double t = a[k * 8 + c]; a[k * 8 + c] = a[p * 8 + c]; a[p * 8 + c] = t; }
            const int t = perm[k]; perm[k] = perm[p]; perm[p] = t;
        }
        for (int r = k + 1; r < 8; ++r) {
            const double l = a[r * 8 + k] / a[k * 8 + k];
            a[r * 8 + k] = l;
            for (int c = k + 1; c < 8; ++c) a[r * 8 + c] = a[r * 8 + c] - l * a[k * 8 + c];
        }
    }
    for (int e = 0; e < 8; ++e) {
        double y[8], x[8];
        for (int i = 0; i < 8; ++i) {
            double s = 0.0;
            for (int j = 0; j < i; ++j) s += a[i * 8 + j] * y[j];
            y[i] = (perm[i] == e ? 1.0 : 0.0) - s;
        }
        for (int i = 7; i >= 0; --i) {
            double s = 0.0;
            for (int j = i + 1; j < 8; ++j) s += a[i * 8 + j] * x[j];
            x[i] = (y[i] - s) / a[i * 8 + i];
        }
        for (int i = 0; i < 8; ++i) {
            if (!finite_d(x[i])) return false;
            hpi[i * 8 + e] = x[i];
        }
    }
    return true;
}

template <class Sync> EDS_HD void marg_frame_body(const MargIo& io, MargMem& m, int tid, int nt, Sync sync) {
    const int N = io.N, nd = N - 8, fo = 4 + 8 * io.frame;
    if (tid == 0) m.bad = 0;
    for (int e = tid; e < N * N; e += nt) m.H[e] = io.HM[(size_t)marg_perm(e / N, fo, nd) * N + marg_perm(e % N, fo, nd)];
    for (int i = tid; i < N; i += nt) m.b[i] = io.bM[marg_perm(i, fo, nd)];
    sync();
    for (int k = tid; k < 8; k += nt) {
        m.H[(nd + k) * N + nd + k] += io.prior[k];
        m.b[nd + k] += io.prior[k] * io.delta_prior[k];
    }
    sync();
    for (int i = tid; i < N; i += nt) {
        const double d = m.H[i * N + i];
        m.S[i] = sqrt((d < 0 ? -d : d) + 10.0);
        m.SI[i] = 1.0 / m.S[i];
    }
    sync();
    for (int e = tid; e < N * N; e += nt) m.H[e] = (m.SI[e / N] * m.H[e]) * m.SI[e % N];
    for (int i = tid; i < N; i += nt) m.b[i] = m.SI[i] * m.b[i];
    sync();
    if (tid == 0) {
        for (int r = 0; r < 8; ++r) for (int c = 0; c < 8; ++c) m.lu[r * 8 + c] = m.H[(nd + r) * N + nd + c];
        if (!inverse8(m.lu, m.hpi)) m.bad = 1;
    }
    sync();
    if (m.bad) {
        if (tid == 0) io.flag[0] = 1;
        return;
    }
    for (int e = tid; e < nd * 8; e += nt) {
        const int i = e / 8, k = e % 8;
        double s = 0.0;
        for (int j = 0; j < 8; ++j) s += m.H[(nd + j) * N + i] * m.hpi[j * 8 + k];
        m.bli[e] = s;
    }
    sync();
    for (int e = tid; e < nd * nd; e += nt) {
        const int i = e / nd, j = e % nd;
        double s = 0.0;
        for (int k = 0; k < 8; ++k) s += m.bli[i * 8 + k] * m.H[(nd + k) * N + j];
        m.H[i * N + j] = m.H[i * N + j] - s;
    }
    for (int i = tid; i < nd; i += nt) {
        double s = 0.0;
        for (int k = 0; k < 8; ++k) s += m.bli[i * 8 + k] * m.b[nd + k];
        m.b[i] = m.b[i] - s;
    }
    sync();
    for (int e = tid; e < nd * nd; e += nt) { const int i = e / nd, j = e % nd; m.H[i * N + j] = (m.S[i] * m.H[i * N + j]) * m.S[j]; }
    for (int i = tid; i < nd; i += nt) m.b[i] = m.S[i] * m.b[i];
    sync();
    for (int e = tid; e < nd * nd; e += nt) {
        const int i = e / nd, j = e % nd;
        if (!finite_d(0.5 * (m.H[i * N + j] + m.H[j * N + i]))) m.bad = 1;
    }
    for (int i = tid; i < nd; i += nt) if (!finite_d(m.b[i])) m.bad = 1;
    sync();
    if (m.bad) {
        if (tid == 0) io.flag[0] = 1;
        return;
    }
    for (int e = tid; e < nd * nd; e += nt) { const int i = e / nd, j = e % nd; io.HM_out[e] = 0.5 * (m.H[i * N + j] + m.H[j * N + i]); }
    for (int i = tid; i < nd; i += nt) io.bM_out[i] = m.b[i];
}
inline void marg_frame_serial(const MargIo& io, MargMem& m) { marg_frame_body(io, m, 0, 1, edsdso::NoSync()); }

// ---- the serial evaluator: what the kernels do, row by row --------------------------------------------------------------------------------
inline void gather_serial(const Cols& narrow, const Cols& wide, const int32_t* map, int rows_new) {
    if (narrow.words) for (int64_t g = 0; g < (int64_t)rows_new * narrow.words; ++g) move_word(narrow, map, g);
    for (int k = 0; k < wide.count; ++k)
        for (int64_t g = 0; g < (int64_t)rows_new * WIDE_PIECES; ++g) move_wide(wide.c[k].src, wide.c[k].dst, map, g);
}

}  // namespace edswed
