// EnergyFunctional::solveSystemF and what stands around it (include/eds_hip_winsolve.h): what the device kernels (eds_winsolve.hip) and
// the host share — setDeltaF's adHTdeltaF, fixLinearizationF, resApprox of modes 1 and 2 of the top accumulator and their per-point
// sums, the assembly of HFinal_top / bFinal_top entry by entry, the scaled LDLT with its substitutions, the orthogonalisation of x,
// resubstituteF's xAd and the point step, setIdepth, calcLEnergyF's per-point value and calcMEnergyF.  fp32 where the reference is
// fp32, fp64 where it is fp64, every sum from 0 in the order written here; every translation unit that includes this is built without
// contraction into FMAs.  Plain C++ outside hipcc.
//
// THE SOLVE.  Not Eigen's code: a stated LDLT of the scaled matrix A = S H S, S = diag(1 / sqrt(H_ii + 10)), of which only the LOWER
// triangle is read (a(i, k) = A(max, min)).  Rows keep their ORIGINAL index r throughout; nothing is swapped.  Step j = 0 ... N - 1:
//   pivot   among the rows not yet taken, the one with the largest |a(r, r) - acc_r|, the LOWEST r on a tie (a NaN never wins);
//           it becomes perm[j], d_j = a(p, p) - acc_p;
//   column  for every row r not yet taken: L(r, j) = (a(r, p) - sum_{k < j} L(r, k) W_k) / d_j with W_k = d_k L(p, k), the sum from 0.0
//           for k = 0 ... j - 1; then acc_r += (L(r, j) d_j) L(r, j).  d_j == 0 exactly: the column is 0.
// so acc_r is the sum over the steps so far, from 0.0 in step order.  Forward substitution y_j = b(perm j) - f, f the sum from 0.0 over
// k = 0 ... j - 1 of L(perm j, k) y_k; z_j = y_j / d_j, or 0 where d_j == 0 (Eigen's solve gives such a component 0 too); backward
// w_j = z_j - g, g the sum from 0.0 over k = N - 1 ... j + 1 (downwards) of L(perm k, j) w_k; x(perm j) = S w_j.  Every sum is taken by
// one thread in that order, so the one-workgroup kernel and the host loop give the same bits.  solve_body is that algorithm ONCE: the
// kernel calls it with its thread index and __syncthreads, the host with one thread and a barrier that does nothing.
#pragma once
#include "eds_window.hpp"

namespace edswsv {

using edswin::J_WORDS;
using edswin::PATTERN;
using edswin::PointOut;

constexpr int MAX_N = 4 + 8 * edswin::MAX_FRAMES;              // 68
// setting_solverMode (reference src/utils/settings.h:35-46)
enum { SOLVER_SVD = 1, SOLVER_ORTHOGONALIZE_SYSTEM = 2, SOLVER_ORTHOGONALIZE_POINTMARG = 4, SOLVER_ORTHOGONALIZE_FULL = 8, SOLVER_SVD_CUT7 = 16,
       SOLVER_REMOVE_POSEPRIOR = 32, SOLVER_USE_GN = 64, SOLVER_FIX_LAMBDA = 128, SOLVER_ORTHOGONALIZE_X = 256, SOLVER_MOMENTUM = 512,
       SOLVER_STEPMOMENTUM = 1024, SOLVER_ORTHOGONALIZE_X_LATER = 2048 };
constexpr int MODE_HONOURED = SOLVER_ORTHOGONALIZE_SYSTEM | SOLVER_USE_GN | SOLVER_FIX_LAMBDA | SOLVER_ORTHOGONALIZE_X | SOLVER_ORTHOGONALIZE_X_LATER |
                              SOLVER_REMOVE_POSEPRIOR;
EDS_HD bool mode_valid(int mode) { return (mode & ~MODE_HONOURED) == 0; }
EDS_HD double mode_lambda(int mode, double lambda) {
    if (mode & SOLVER_USE_GN) lambda = 0;
    if (mode & SOLVER_FIX_LAMBDA) lambda = 1e-5;
    return lambda;
}
EDS_HD bool mode_orth_x(int mode, int iteration) { return (mode & SOLVER_ORTHOGONALIZE_X) || (iteration >= 2 && (mode & SOLVER_ORTHOGONALIZE_X_LATER)); }
EDS_HD bool finite_d(double v) { return v - v == 0.0; }

// ---- setDeltaF (EnergyFunctional.cpp:171-194) ---------------------------------------------------------------------------------------------
// adHTdeltaF[h + F t][j] = sum_k (float)delta_h[k] adHostF(k, j), from 0 with k = 0 ... 7, the same for the target, the two added
EDS_HD void adht_delta(const float* adHostF, const float* adTargetF, const double* delta_h, const double* delta_t, float* out) {
    for (int j = 0; j < 8; ++j) {
        float a = 0, b = 0;
        for (int k = 0; k < 8; ++k) a += (float)delta_h[k] * adHostF[8 * k + j];
        for (int k = 0; k < 8; ++k) b += (float)delta_t[k] * adTargetF[8 * k + j];
        out[j] = a + b;
    }
}

// ---- fixLinearizationF (EnergyFunctionalStructs.cpp:87-113), mode 1's resApprox (AccumulatedTopHessian.cpp:78-96) --------------------------
// Jp_delta of row q (0: x, 1: y): the 6-term dot, the 4-term dot, the Jpdd product, each dot from 0 in index order, added left to right
EDS_HD float jp_delta(const float* J, int q, const float* dp, const float* dc, float dd) {
    float a = 0, b = 0;
    for (int i = 0; i < 6; ++i) a += J[edswin::J_JPDXI + 6 * q + i] * dp[i];
    for (int i = 0; i < 4; ++i) b += J[edswin::J_JPDC + 4 * q + i] * dc[i];
    return (a + b) + J[edswin::J_JPDD + q] * dd;
}
EDS_HD float rtz_tap(const float* J, int i, float jx, float jy, float da, float db) {
    return (((J[edswin::J_RESF + i] - J[edswin::J_JIDX + i] * jx) - J[edswin::J_JIDX + 8 + i] * jy) - J[edswin::J_JABF + i] * da) - J[edswin::J_JABF + 8 + i] * db;
}
EDS_HD float approx_tap(const float* J, float rtz, int i, float jx, float jy, float da, float db) {
    return (((rtz + J[edswin::J_JIDX + i] * jx) + J[edswin::J_JIDX + 8 + i] * jy) + J[edswin::J_JABF + i] * da) + J[edswin::J_JABF + 8 + i] * db;
}
// calcLEnergyPt's term of one tap (EnergyFunctional.cpp:366-379): Jdelta ((rtz + rtz) + Jdelta)
EDS_HD float lenergy_tap(const float* J, float rtz, int i, float jx, float jy, float da, float db) {
    const float jd = ((J[edswin::J_JIDX + i] * jx + J[edswin::J_JIDX + 8 + i] * jy) + J[edswin::J_JABF + i] * da) + J[edswin::J_JABF + 8 + i] * db;
    return jd * ((rtz + rtz) + jd);
}

// what the per-residual and per-point functions read
struct Lin {
    int32_t F;
    const int32_t *res_first, *res_point, *res_target, *active, *lin;
    const edswin::Point* pts;
    const float *efJ, *rtz, *res_approx, *adHTdeltaF, *cDeltaF, *deltaF, *priorF;
};

// one tap of one residual: fixLinearizationF's res_toZeroF, and resApprox of mode 1 (2: res_toZeroF itself)
EDS_HD void res_deltas(const Lin& t, int r, float* jx, float* jy, const float** dp) {
    const int p = t.res_point[r];
    const float* J = t.efJ + (size_t)r * J_WORDS;
    *dp = t.adHTdeltaF + (size_t)(t.pts[p].host + t.F * t.res_target[r]) * 8;
    *jx = jp_delta(J, 0, *dp, t.cDeltaF, t.deltaF[p]);
    *jy = jp_delta(J, 1, *dp, t.cDeltaF, t.deltaF[p]);
}
EDS_HD float fix_tap(const Lin& t, int r, int i) {
    float jx, jy;
    const float* dp;
    res_deltas(t, r, &jx, &jy, &dp);
    return rtz_tap(t.efJ + (size_t)r * J_WORDS, i, jx, jy, dp[6], dp[7]);
}
EDS_HD float res_approx_tap(const Lin& t, int mode, int r, int i) {
    const float rtz = t.rtz[(size_t)r * PATTERN + i];
    if (mode != 1) return rtz;
    float jx, jy;
    const float* dp;
    res_deltas(t, r, &jx, &jy, &dp);
    return approx_tap(t.efJ + (size_t)r * J_WORDS, rtz, i, jx, jy, dp[6], dp[7]);
}

// the sums addPoint<1> / <2> leave in Hdd_accLF, bd_accLF, Hcd_accLF[4] (out[0 .. 5]), residuals in table order; returns the residuals added
EDS_HD int lf_sums(const Lin& t, int mode, int p, float* out) {
    float bd = 0, Hdd = 0, Hcd[4] = {0, 0, 0, 0};
    int n = 0;
    for (int r = t.res_first[p]; r < t.res_first[p + 1]; ++r) {
        if (!edswin::top_filter(mode, t.active[r], t.lin[r])) continue;
        edswin::top_point_term(t.efJ + (size_t)r * J_WORDS, t.res_approx + (size_t)r * PATTERN, bd, Hdd, Hcd);
        ++n;
    }
    out[0] = Hdd; out[1] = bd;
    for (int k = 0; k < 4; ++k) out[2 + k] = Hcd[k];
    return n;
}

// calcLEnergyPt for one point, in fp64 from 0.0: its linearized active residuals in table order, taps 0 ... 7, then deltaF deltaF priorF
EDS_HD double lenergy_point(const Lin& t, int p) {
    double e = 0.0;
    const float dd = t.deltaF[p];
    const int host = t.pts[p].host;
    for (int r = t.res_first[p]; r < t.res_first[p + 1]; ++r) {
        if (!t.lin[r] || !t.active[r]) continue;
        const float* J = t.efJ + (size_t)r * J_WORDS;
        const float* dp = t.adHTdeltaF + (size_t)(host + t.F * t.res_target[r]) * 8;
        const float jx = jp_delta(J, 0, dp, t.cDeltaF, dd), jy = jp_delta(J, 1, dp, t.cDeltaF, dd);
        for (int i = 0; i < PATTERN; ++i) e += (double)lenergy_tap(J, t.rtz[(size_t)r * PATTERN + i], i, jx, jy, dp[6], dp[7]);
    }
    e += (double)(dd * dd * t.priorF[p]);
    return e;
}
// the frames' and the calibration's prior terms of calcLEnergyF_MT (EnergyFunctional.cpp:398-403): vec = delta[68], prior[68],
// prior * delta_prior[68], delta_prior[68] with the calibration in 0 ... 3; cF = cDeltaF[4], cPriorF[4]
EDS_HD double lenergy_priors(int F, const double* vec, const float* cF) {
    double E = 0;
    for (int f = 0; f < F; ++f) {
        double d = 0.0;
        for (int k = 0; k < 8; ++k) d += (vec[3 * MAX_N + 4 + 8 * f + k] * vec[MAX_N + 4 + 8 * f + k]) * vec[3 * MAX_N + 4 + 8 * f + k];
        E += d;
    }
    float c = 0;
    for (int k = 0; k < 4; ++k) c += (cF[k] * cF[4 + k]) * cF[k];
    E += c;
    return E;
}

// calcMEnergyF: delta . (2 bM + HM delta), every row and the final dot from 0.0 in index order
EDS_HD double menergy_row(int N, const double* HM, const double* bM, const double* delta, int i) {
    double v = 0.0;
    for (int j = 0; j < N; ++j) v += HM[(size_t)i * N + j] * delta[j];
    return 2 * bM[i] + v;
}

// ---- the assembly of solveSystemF (EnergyFunctional.cpp:798-850), one entry at a time --------------------------------------------------------
// work: the solve's matrices on the device, N N each unless noted, in this order
enum { W_HM = 0, W_P, W_HT, W_T1, W_T2, W_HF, W_LASTH, W_MATS };
enum { V_BM = 0, V_BT, V_TB, V_BF, V_LASTB, V_X, V_BMTOP, V_VECS };
EDS_HD int work_words() { return W_MATS * MAX_N * MAX_N + V_VECS * MAX_N; }
struct Sys {
    int32_t N, system, orth_system;
    double lambda;
    const double *HA, *bA, *Hsc, *bsc;                          // both stitches of mode 0 and the Schur complement
    const double *HL, *bL;                                      // mode 1's stitch, before the priors
    const double* vec;                                          // delta, prior, prior * delta_prior, delta_prior
    double* work;
    EDS_HD double* mat(int k) const { return work + (size_t)k * MAX_N * MAX_N; }
    EDS_HD double* v(int k) const { return work + (size_t)W_MATS * MAX_N * MAX_N + (size_t)k * MAX_N; }
};
// stage 0: entry e < N N is (i, j), e >= N N is row i of the right-hand side.  H_L and b_L get usePrior's adds (AccumulatedTopHessian.cpp:
// 227-237) here, after the stitch.  Without SOLVER_ORTHOGONALIZE_SYSTEM this finishes HFinal_top, bFinal_top, lastHS, lastbS; with it, it
// leaves HT_act, bT_act.  stages 1 and 2 (only when the system is orthogonalised): T1 = P HT, tb = P bT; T2 = T1 P.  stage 3: the rest of
// the SYSTEM branch.  Every statement adds left to right as the reference writes it.
EDS_HD void assemble(const Sys& s, int stage, int e) {
    const int N = s.N;
    const bool vecrow = e >= N * N;
    const int i = vecrow ? e - N * N : e / N, j = vecrow ? 0 : e % N;
    const double *HM = s.mat(W_HM), *P = s.mat(W_P), *bM = s.v(V_BM);
    if (stage == 0) {
        if (vecrow) {
            const double bL = s.bL[i] + s.vec[2 * MAX_N + i];
            double t = 0.0;
            for (int k = 0; k < N; ++k) t += HM[(size_t)i * N + k] * s.vec[k];
            const double bMtop = bM[i] + t;
            s.v(V_BMTOP)[i] = bMtop;
            if (s.system) s.v(V_BT)[i] = (bL + s.bA[i]) - s.bsc[i];
            else { const double b = ((bL + bMtop) + s.bA[i]) - s.bsc[i]; s.v(V_BF)[i] = b; s.v(V_LASTB)[i] = b; }
            return;
        }
        double HL = s.HL[e];
        if (i == j) HL += s.vec[MAX_N + i];
        if (s.system) { s.mat(W_HT)[e] = (HL + s.HA[e]) - s.Hsc[e]; return; }
        double Hf = (HL + HM[e]) + s.HA[e];
        s.mat(W_LASTH)[e] = Hf - s.Hsc[e];
        if (i == j) Hf *= (1 + s.lambda);
        s.mat(W_HF)[e] = Hf - s.Hsc[e] * (1.0f / (1 + s.lambda));
        return;
    }
    if (stage == 1) {
        double t = 0.0;
        if (vecrow) { for (int k = 0; k < N; ++k) t += P[(size_t)i * N + k] * s.v(V_BT)[k]; s.v(V_TB)[i] = t; }
        else { for (int k = 0; k < N; ++k) t += P[(size_t)i * N + k] * s.mat(W_HT)[(size_t)k * N + j]; s.mat(W_T1)[e] = t; }
        return;
    }
    if (stage == 2) {
        if (vecrow) return;
        double t = 0.0;
        for (int k = 0; k < N; ++k) t += s.mat(W_T1)[(size_t)i * N + k] * P[(size_t)k * N + j];
        s.mat(W_T2)[e] = t;
        return;
    }
    if (vecrow) {
        double bT = s.v(V_BT)[i];
        if (s.orth_system) bT -= s.v(V_TB)[i];
        const double b = bT + s.v(V_BMTOP)[i];
        s.v(V_BF)[i] = b; s.v(V_LASTB)[i] = b;
        return;
    }
    double HT = s.mat(W_HT)[e];
    if (s.orth_system) HT -= s.mat(W_T2)[e];
    double Hf = HT + HM[e];
    s.mat(W_LASTH)[e] = Hf;
    if (i == j) Hf *= (1 + s.lambda);
    s.mat(W_HF)[e] = Hf;
}

// ---- the solve, the orthogonalisation of x and resubstituteF's xAd: ONE workgroup, or one host thread ------------------------------------
// the arrays a workgroup keeps in LDS: about 60 kB
struct SolveMem {
    double L[MAX_N * MAX_N], A[MAX_N * (MAX_N + 1) / 2], S[MAX_N], y[MAX_N], acc[MAX_N], dg[MAX_N], W[MAX_N], w[MAX_N], x[MAX_N];
    int32_t perm[MAX_N], pos[MAX_N], bad;
};
EDS_HD int tri(int r, int k) { return r >= k ? r * (r + 1) / 2 + k : k * (k + 1) / 2 + r; }

struct SolveIo {
    int32_t N, F, orth_x;
    const double *H, *b, *P;                                    // HFinal_top, bFinal_top, the projector (read when orth_x)
    const float* adF;                                           // adHostF then adTargetF, [h + F t][8][8] each
    double* x;                                                  // N
    float* xAd;                                                 // [F h + t][8], then cstep[4]
    int32_t* flag;                                              // flag[0] = 1 when x is not finite (then xAd is not written)
    double *L_out, *d_out;                                      // may be NULL: the factors, L (N N, row r, step j), d then perm as doubles (2 N)
};

template <class Sync> EDS_HD void solve_body(const SolveIo& io, SolveMem& m, int tid, int nt, Sync sync) {
    const int N = io.N;
    for (int r = tid; r < N; r += nt) m.S[r] = 1.0 / sqrt(io.H[(size_t)r * N + r] + 10.0);
    sync();
    for (int r = tid; r < N; r += nt) {
        for (int k = 0; k <= r; ++k) m.A[tri(r, k)] = (m.S[r] * io.H[(size_t)r * N + k]) * m.S[k];
        m.y[r] = m.S[r] * io.b[r];
        m.acc[r] = 0.0;
        m.pos[r] = N;
        for (int k = 0; k < N; ++k) m.L[r * MAX_N + k] = 0.0;
    }
    sync();
    for (int j = 0; j < N; ++j) {
        if (tid == 0) {
            int p = -1;
            double best = 0.0;
            for (int r = 0; r < N; ++r) {
                if (m.pos[r] < N) continue;
                const double v = fabs(m.A[tri(r, r)] - m.acc[r]);
                if (p < 0 || v > best) { p = r; best = v; }
            }
            m.perm[j] = p; m.pos[p] = j; m.dg[j] = m.A[tri(p, p)] - m.acc[p];
        }
        sync();
        const int p = m.perm[j];
        const double d = m.dg[j];
        for (int k = tid; k < j; k += nt) m.W[k] = m.dg[k] * m.L[p * MAX_N + k];
        sync();
        for (int r = tid; r < N; r += nt) {
            if (m.pos[r] < N) continue;
            double s = 0.0;
            for (int k = 0; k < j; ++k) s += m.L[r * MAX_N + k] * m.W[k];
            const double l = d == 0.0 ? 0.0 : (m.A[tri(r, p)] - s) / d;
            m.L[r * MAX_N + j] = l;
            m.acc[r] += (l * d) * l;
        }
        sync();
    }
    // forward: acc_r restarts as the running sum f of row r
    for (int r = tid; r < N; r += nt) m.acc[r] = 0.0;
    sync();
    for (int k = 0; k < N; ++k) {
        if (tid == 0) { const int p = m.perm[k]; m.w[k] = m.y[p] - m.acc[p]; }
        sync();
        for (int r = tid; r < N; r += nt) if (m.pos[r] > k) m.acc[r] += m.L[r * MAX_N + k] * m.w[k];
        sync();
    }
    for (int k = tid; k < N; k += nt) { m.w[k] = m.dg[k] == 0.0 ? 0.0 : m.w[k] / m.dg[k]; m.W[k] = 0.0; }
    sync();
    // backward: W_j is the running sum g of step j
    for (int k = N - 1; k >= 0; --k) {
        if (tid == 0) m.w[k] = m.w[k] - m.W[k];
        sync();
        for (int j = tid; j < k; j += nt) m.W[j] += m.L[m.perm[k] * MAX_N + j] * m.w[k];
        sync();
    }
    for (int k = tid; k < N; k += nt) { const int p = m.perm[k]; m.x[p] = m.S[p] * m.w[k]; }
    sync();
    if (io.orth_x) {                                            // x -= P x, rows summed in index order
        for (int r = tid; r < N; r += nt) {
            double t = 0.0;
            for (int k = 0; k < N; ++k) t += io.P[(size_t)r * N + k] * m.x[k];
            m.y[r] = t;
        }
        sync();
        for (int r = tid; r < N; r += nt) m.x[r] = m.x[r] - m.y[r];
        sync();
    }
    if (tid == 0) {
        int bad = 0;
        for (int r = 0; r < N; ++r) if (!finite_d(m.x[r])) bad = 1;
        m.bad = bad;
        io.flag[0] = bad;
    }
    sync();
    for (int r = tid; r < N; r += nt) {
        io.x[r] = m.x[r];
        if (io.d_out) { io.d_out[r] = m.dg[r]; io.d_out[N + r] = (double)m.perm[r]; }
        if (io.L_out) for (int k = 0; k < N; ++k) io.L_out[(size_t)r * N + k] = m.L[r * MAX_N + k];
    }
    if (m.bad) return;
    // resubstituteF_MT (EnergyFunctional.cpp:263-282): xF = (float)x; xAd[F h + t] = xF_h^T adHostF[h + F t] + xF_t^T adTargetF[h + F t]
    const int F = io.F;
    for (int e = tid; e < F * F * 8; e += nt) {
        const int q = e >> 3, jj = e & 7, h = q / F, t = q % F;
        const float *AH = io.adF + (size_t)(h + F * t) * 64, *AT = io.adF + (size_t)F * F * 64 + (size_t)(h + F * t) * 64;
        float a = 0, b = 0;
        for (int k = 0; k < 8; ++k) a += (float)m.x[4 + 8 * h + k] * AH[8 * k + jj];
        for (int k = 0; k < 8; ++k) b += (float)m.x[4 + 8 * t + k] * AT[8 * k + jj];
        io.xAd[e] = a + b;
    }
    for (int k = tid; k < 4; k += nt) io.xAd[F * F * 8 + k] = (float)m.x[k];
}

// ---- resubstituteFPt (EnergyFunctional.cpp:284-317) and setIdepth (HessianBlocks.h:445-448) ---------------------------------------------------
// xAd: [F host + target][8] then cstep[4]; lf: the point's six linearized sums (Hcd_accLF is lf[2 .. 5])
EDS_HD float point_step(const Lin& t, const PointOut& o, const float* lf, const float* JpJdF, const float* xAd, int p) {
    if (o.nres == 0) return 0.0f;
    const float* xc = xAd + t.F * t.F * 8;
    float b = o.bdSumF;
    float s = 0;
    for (int k = 0; k < 4; ++k) s += xc[k] * (o.Hcd_accAF[k] + lf[2 + k]);
    b -= s;
    const int host = t.pts[p].host;
    for (int r = t.res_first[p]; r < t.res_first[p + 1]; ++r) {
        if (!t.active[r]) continue;
        const float* xa = xAd + (size_t)(t.F * host + t.res_target[r]) * 8;
        float d = 0;
        for (int k = 0; k < 8; ++k) d += xa[k] * JpJdF[(size_t)r * 8 + k];
        b -= d;
    }
    return -b * o.HdiF;
}
// idepth = SCALE_IDEPTH_INVERSE idepth_scaled (setIdepthScaled), and back after the step
EDS_HD float idepth_of(float idepth_scaled, float scale_idepth) { return (1.0f / scale_idepth) * idepth_scaled; }
// setDeltaF's per-point line (EnergyFunctional.cpp:190): deltaF = idepth - idepth_zero, each the scaled value times 1 / SCALE_IDEPTH
EDS_HD float delta_of_idepths(float idepth_scaled, float idepth_zero_scaled, float scale_idepth) {
    const float inv = 1.0f / scale_idepth;
    return inv * idepth_scaled - inv * idepth_zero_scaled;
}
EDS_HD float stepped_idepth_scaled(float backup, float fac, float step, float scale_idepth) { return scale_idepth * (backup + fac * step); }

#if !defined(__HIP_DEVICE_COMPILE__)
inline void solve_serial(const SolveIo& io, SolveMem& m) { solve_body(io, m, 0, 1, edsdso::NoSync()); }
#endif

}  // namespace edswsv
