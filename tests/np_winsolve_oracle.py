"""numpy restatement, from the reference's text, of what include/eds_hip_winsolve.h adds to the window: setDeltaF's adHTdeltaF
(EnergyFunctional.cpp:171-194), fixLinearizationF (EnergyFunctionalStructs.cpp:87-113), resApprox and the per-point sums of
addPoint<1> (AccumulatedTopHessian.cpp:40-159), the Schur prologue's bdSumF, the assembly of solveSystemF (EnergyFunctional.cpp:798-850)
with stitchDouble's priors (AccumulatedTopHessian.cpp:227-237), resubstituteF_MT's xAd and resubstituteFPt's step (:263-317), setIdepth,
calcLEnergyF_MT's terms (:332-413) and calcMEnergyF.  fp32 in the operand order the issue states, one numpy operation per rounding.
The window's own per-residual arithmetic (the functional's J, JpJdF, the active flags, mode 0's sums) is tests/np_window_oracle.py's;
here it is an input, read from the host window.  Every `mut` names one deliberate mistake (tests/test_winsolve_oracle.py)."""
import math

import numpy as np

import np_window_oracle as no

f32 = np.float32
J_RESF, J_JPDXI, J_JPDC, J_JPDD, J_JIDX, J_JABF, J_JIDX2 = 0, 8, 20, 28, 30, 46, 62


def ulps(a, b):
    """distance of two fp32 values in units in the last place of the larger"""
    a, b = f32(a), f32(b)
    return abs(float(a) - float(b)) / float(np.spacing(max(abs(a), abs(b), f32(1e-37))))


def adht_delta(F, adH, adT, delta, mut=None):
    """adHTdeltaF[h + F t][j] = sum_k (float)delta_h[k] adHostF(k, j) from 0, the same for the target, the two added"""
    adHF, adTF, d = adH.astype(f32), adT.astype(f32), delta.astype(f32)
    out = np.zeros((F * F, 8), f32)
    for h in range(F):
        for t in range(F):
            idx = h + F * t
            src = F * h + t if mut == "adHostF_index" else idx
            a, b = np.zeros(8, f32), np.zeros(8, f32)
            for k in range(8):
                a = a + d[h, k] * adHF[src, k, :]
            for k in range(8):
                b = b + d[t, k] * adTF[idx, k, :]
            out[idx] = a + b
    return out


class Tables:
    """what the host window holds after linearize -> apply, and the state of eds_wsv_set_state"""

    def __init__(self, s, residuals, is_linearized):
        c = s.win
        self.s, self.F, self.n, self.m = s, s.F, s.n, s.m
        self.J, self.active, self.JpJdF = residuals["ef_J"], residuals["is_active"] != 0, residuals["JpJdF"]
        self.lin = np.asarray(is_linearized) != 0
        self.point, self.target, self.host = c.point, c.target, c.host
        self.res_host = c.host[c.point] if s.m else np.zeros(0, np.int32)
        self.first = np.searchsorted(c.point, np.arange(s.n + 1)).astype(int)
        self.cDeltaF = s.cDelta.astype(f32)
        self.priorF, self.deltaF = np.asarray(s.priorF, f32).copy(), np.asarray(s.deltaF, f32)


def jp_delta(T, adht, mut=None):
    """per residual: Jp_delta_x, Jp_delta_y (the 6-term dot, the 4-term dot, the Jpdd product, left to right), delta_a, delta_b"""
    dp = adht[T.res_host + T.F * T.target]
    dd = T.deltaF[T.point]
    out = []
    for q in range(2):
        a, b = np.zeros(T.m, f32), np.zeros(T.m, f32)
        for i in range(6):
            a = a + T.J[:, J_JPDXI + 6 * q + i] * dp[:, i]
        for i in range(4):
            b = b + T.J[:, J_JPDC + 4 * q + i] * T.cDeltaF[i]
        out.append((a + b) + T.J[:, J_JPDD + q] * dd)
    return out[0], out[1], dp[:, 6], dp[:, 7]


def fix_linearization(T, adht, mut=None):
    """res_toZeroF of every residual (the caller keeps the selected ones)"""
    jx, jy, da, db = (v[:, None] for v in jp_delta(T, adht))
    J = T.J
    r = J[:, J_RESF:J_RESF + 8] - J[:, J_JIDX:J_JIDX + 8] * jx
    r = r + J[:, J_JIDX + 8:J_JIDX + 16] * jy if mut == "fix_sign" else r - J[:, J_JIDX + 8:J_JIDX + 16] * jy
    r = r - J[:, J_JABF:J_JABF + 8] * da
    return (r - J[:, J_JABF + 8:J_JABF + 16] * db).astype(f32)


def res_approx(T, adht, rtz):
    """mode 1: res_toZeroF plus the four products in the reference's order"""
    jx, jy, da, db = (v[:, None] for v in jp_delta(T, adht))
    J = T.J
    r = rtz + J[:, J_JIDX:J_JIDX + 8] * jx
    r = r + J[:, J_JIDX + 8:J_JIDX + 16] * jy
    r = r + J[:, J_JABF:J_JABF + 8] * da
    return (r + J[:, J_JABF + 8:J_JABF + 16] * db).astype(f32)


def lf_sums(T, approx, take):
    """Hdd_accLF, bd_accLF, Hcd_accLF[4] per point over the residuals with take[r], in table order"""
    J = T.J
    jr0, jr1 = np.zeros(T.m, f32), np.zeros(T.m, f32)
    for i in range(8):
        jr0 = jr0 + approx[:, i] * J[:, J_JIDX + i]
        jr1 = jr1 + approx[:, i] * J[:, J_JIDX + 8 + i]
    d0, d1 = J[:, J_JPDD], J[:, J_JPDD + 1]
    q0 = J[:, J_JIDX2] * d0 + J[:, J_JIDX2 + 1] * d1
    q1 = J[:, J_JIDX2 + 2] * d0 + J[:, J_JIDX2 + 3] * d1
    bd_t, Hdd_t = jr0 * d0 + jr1 * d1, q0 * d0 + q1 * d1
    Hcd_t = J[:, J_JPDC:J_JPDC + 4] * q0[:, None] + J[:, J_JPDC + 4:J_JPDC + 8] * q1[:, None]
    out = np.zeros((T.n, 6), f32)
    for r in np.nonzero(take)[0]:
        p = T.point[r]
        out[p, 0] = out[p, 0] + Hdd_t[r]
        out[p, 1] = out[p, 1] + bd_t[r]
        out[p, 2:] = out[p, 2:] + Hcd_t[r]
    return out


def schur_prologue(T, pts, lf, shift=True):
    """HdiF and bdSumF of AccumulatedSCHessianSSE::addPoint from the A sums, the L sums and the prior; also how many H < 1e-10
    decisions lie within 4 ulps of flipping"""
    H = (pts["Hdd_accAF"] + lf[:, 0]) + T.priorF
    live = pts["nres"] > 0
    undecided = int(sum(1 for p in np.nonzero(live)[0] if ulps(H[p], 1e-10) <= 4))
    H = np.where(H < 1e-10, f32(1e-10), H).astype(f32)
    hdi = (1.0 / H.astype(np.float64)).astype(f32)
    bds = pts["bd_accAF"] + lf[:, 1]
    if shift:
        bds = bds + T.priorF * T.deltaF
    return np.where(live, hdi, f32(0)).astype(f32), np.where(live, bds, f32(0)).astype(f32), undecided


def top_acc_exact(T, approx, take):
    """mode 1's top accumulators: math.fsum of the fp32 terms per word, and n 2^-53 sum|term| with n the points of the word's host"""
    F = T.F
    size = F * F * no.TOP_WORDS
    terms = [[] for _ in range(size)]
    idx = np.nonzero(take)[0]
    J = T.J[idx].copy()
    J[:, J_RESF:J_RESF + 8] = approx[idx]
    tt = no.top_terms(J)
    for k, r in enumerate(idx):
        base = (int(T.res_host[r]) + F * int(T.target[r])) * no.TOP_WORDS
        for e in range(91):
            terms[base + e].append(float(tt[k, e]))
        terms[base + 91].append(1.0)
    counts = np.bincount(T.host, minlength=F).astype(np.float64)
    n_of = counts[(np.arange(size) // no.TOP_WORDS) % F]
    acc = np.array([math.fsum(t) for t in terms])
    absum = np.array([math.fsum(abs(v) for v in t) for t in terms])
    return acc, absum * n_of * 2.0 ** -53


def stitched_delta(s):
    return np.concatenate([s.cDelta.astype(f32).astype(np.float64), s.delta.ravel()])


def rows_times(M, v):
    """M v, every row summed from 0 in index order"""
    out = np.zeros(len(v))
    for j in range(len(v)):
        out = out + M[:, j] * v[j]
    return out


def assemble(s, r, raw, HM, bM, mut=None):
    """HFinal_top, bFinal_top, lastHS, lastbS of one round from the stitched matrices, added left to right as the statements are written"""
    N = s.N
    lam = 0.0 if r.mode & 64 else r.lam
    lam = 1e-5 if r.mode & 128 else lam
    prior = np.concatenate([s.cPrior, s.prior.ravel()])
    dp = s.delta if mut == "prior_delta" else s.delta_prior
    pdp = np.concatenate([s.cPrior * s.cDelta.astype(f32).astype(np.float64), (s.prior * dp).ravel()])
    HL = raw["H_L"] + np.diag(prior)
    HL[~np.eye(N, dtype=bool)] = raw["H_L"][~np.eye(N, dtype=bool)]            # only the diagonal receives an addition
    bL = raw["b_L"] + pdp
    bMtop = bM + rows_times(HM, stitched_delta(s))
    P = s.P if r.use_p else None
    if r.mode & 2:
        HT = (HL + raw["H_A"]) - raw["H_sc"]
        bT = (bL + raw["b_A"]) - raw["b_sc"]
        if not r.hff and P is not None:
            T1 = np.zeros((N, N))
            for k in range(N):
                T1 = T1 + np.outer(P[:, k], HT[k, :])
            T2 = np.zeros((N, N))
            for k in range(N):
                T2 = T2 + np.outer(T1[:, k], P[k, :])
            bT = bT - rows_times(P, bT)
            HT = HT - T2
        Hf, bf = HT + HM, bT + bMtop
        lastH, lastb = Hf.copy(), bf.copy()
        Hf[np.diag_indices(N)] = np.diag(Hf) * (1 + lam)
    else:
        Hf = (HL + HM) + raw["H_A"]
        bf = ((bL + bMtop) + raw["b_A"]) - raw["b_sc"]
        lastH, lastb = Hf - raw["H_sc"], bf.copy()
        Hf[np.diag_indices(N)] = np.diag(Hf) * (1 + lam)
        Hf = Hf - (raw["H_sc"] if mut == "no_divisor" else raw["H_sc"] * (1.0 / (1 + lam)))
    return Hf, bf, lastH, lastb


def x_ad(s, x, adH, adT, mut=None):
    """xAd[F h + t] = xF_h^T adHostF[h + F t] + xF_t^T adTargetF[h + F t]; returns it indexed [F h + t]"""
    F = s.F
    xF, adHF, adTF = x.astype(f32), adH.astype(f32), adT.astype(f32)
    out = np.zeros((F * F, 8), f32)
    for h in range(F):
        for t in range(F):
            a, b = np.zeros(8, f32), np.zeros(8, f32)
            for k in range(8):
                a = a + xF[4 + 8 * h + k] * adHF[h + F * t, k, :]
            for k in range(8):
                b = b + xF[4 + 8 * t + k] * adTF[h + F * t, k, :]
            out[h + F * t if mut == "xAd_index" else F * h + t] = a + b
    return out


def steps(T, pts, lf, xAd, x, hdi=None, bds=None):
    """resubstituteFPt: b = bdSumF; subtract the 4-term dot with Hcd_accAF + Hcd_accLF; for every active residual in table order
    subtract the 8-term dot of xAd with JpJdF; step = -b HdiF; 0 when the point has no active residual"""
    xc = x[:4].astype(f32)
    hdi = pts["HdiF"] if hdi is None else hdi
    bds = pts["bdSumF"] if bds is None else bds
    out = np.zeros(T.n, f32)
    for p in range(T.n):
        rs = [r for r in range(T.first[p], T.first[p + 1]) if T.active[r]]
        if not rs:
            continue
        b = f32(bds[p])
        d = f32(0)
        for k in range(4):
            d = d + xc[k] * (pts["Hcd_accAF"][p, k] + lf[p, 2 + k])
        b = b - d
        for r in rs:
            xa = xAd[T.F * T.host[p] + T.target[r]]
            d = f32(0)
            for k in range(8):
                d = d + xa[k] * T.JpJdF[r, k]
            b = b - d
        out[p] = -b * hdi[p]
    return out


def stepped(ids_backup_scaled, fac, step, scale=1.0):
    """setIdepth(idepth_backup + fac step): idepth_scaled = SCALE_IDEPTH idepth"""
    backup = (f32(1.0) / f32(scale)) * ids_backup_scaled
    return (f32(scale) * (backup + f32(fac) * step)).astype(f32)


def l_energy_terms(T, adht, rtz):
    """per point the fp32 terms of calcLEnergyPt in order: linearized active residuals in table order, taps 0 ... 7, then the prior term"""
    jx, jy, da, db = (v[:, None] for v in jp_delta(T, adht))
    J = T.J
    jd = ((J[:, J_JIDX:J_JIDX + 8] * jx + J[:, J_JIDX + 8:J_JIDX + 16] * jy) + J[:, J_JABF:J_JABF + 8] * da) + J[:, J_JABF + 8:J_JABF + 16] * db
    term = (jd * ((rtz + rtz) + jd)).astype(f32)
    take = T.lin & T.active
    out = []
    for p in range(T.n):
        t = [float(v) for r in range(T.first[p], T.first[p + 1]) if take[r] for v in term[r]]
        t.append(float(T.deltaF[p] * T.deltaF[p] * T.priorF[p]))
        out.append(t)
    return out


def l_energy_priors(s):
    E = 0.0
    for f in range(s.F):
        d = 0.0
        for k in range(8):
            d += (s.delta_prior[f, k] * s.prior[f, k]) * s.delta_prior[f, k]
        E += d
    cd, cp = s.cDelta.astype(f32), s.cPrior.astype(f32)
    c = f32(0)
    for k in range(4):
        c = c + (cd[k] * cp[k]) * cd[k]
    return E + float(c)


def m_energy_terms(s, HM, bM):
    """the N products delta_i (2 bM_i + (HM delta)_i) and every product under them, for the exact value and the bound"""
    d = stitched_delta(s)
    exact = math.fsum(d[i] * (2 * bM[i] + math.fsum(HM[i, j] * d[j] for j in range(s.N))) for i in range(s.N))
    mag = math.fsum(abs(d[i]) * (2 * abs(bM[i]) + math.fsum(abs(HM[i, j] * d[j]) for j in range(s.N))) for i in range(s.N))
    return exact, mag


def ldlt_check(H, b, x_hat_scaled, L, d, perm):
    """the componentwise backward bound of the scaled system: |b^ - A^ x^| <= gamma_{3 N + 1} (|L||D||L^T|) |x^| with the restatement's
    factors (Higham, Accuracy and Stability, Theorem 10.4 for the factorisation and 8.5 for the substitutions), in the pivoted order.
    The residual is evaluated exactly, in rational arithmetic, so that its own rounding does not enter; returns (largest fraction of
    the bound, the bound as a vector, pivot choices within 4 ulps of a tie)"""
    from fractions import Fraction
    N = len(b)
    S = 1.0 / np.sqrt(np.diag(H) + 10.0)
    A = np.tril((S[:, None] * H) * S[None, :])
    A = A + np.tril(A, -1).T                                     # the lower triangle is what is read
    bh = S * b
    Lp = np.eye(N)
    for j in range(N):
        for k in range(j):
            Lp[j, k] = L[perm[j], k]
    Ap, bp, xp = A[np.ix_(perm, perm)], bh[perm], x_hat_scaled[perm]
    u = 2.0 ** -53
    g = (3 * N + 1) * u / (1 - (3 * N + 1) * u)
    bound = g * (np.abs(Lp) @ np.diag(np.abs(d)) @ np.abs(Lp).T) @ np.abs(xp)
    xq = [Fraction(float(v)) for v in xp]
    resid = np.array([float(abs(Fraction(float(bp[i])) - sum(Fraction(float(Ap[i, j])) * xq[j] for j in range(N)))) for i in range(N)])
    frac = float(np.max(resid / bound))
    # ties: the diagonal of the trailing block when step j picked its pivot
    ties = 0
    acc = np.zeros(N)
    taken = np.zeros(N, bool)
    for j in range(N):
        p = perm[j]
        cand = np.abs(np.diag(A) - acc)
        best = cand[p]
        for r in np.nonzero(~taken)[0]:
            if r != p and abs(cand[r] - best) <= 4 * np.spacing(best):
                ties += 1
        taken[p] = True
        acc = acc + (L[:, j] * d[j]) * L[:, j]
    return frac, bound, ties


def orth_system_bound(s, raw, HLb, bLb, lam, HM, bM):
    """the entrywise bound of the orthogonalised SYSTEM branch between two evaluations of the statements, one on H_L, b_L that are off
    by at most HLb, bLb.  With E0 = HLb + 3 u (|H_L| + prior + |H_A| + |H_sc|) the distance of the two HT_act and
    Q = |P| |HT| |P|: the two N-term dot products per entry of (P HT) P cost gamma_{2 N} Q in each evaluation, the input's distance
    passes through as |P| E0 |P|, and the subtraction, the HM add and the (1 + lambda) scaling are three more roundings."""
    N, u = s.N, 2.0 ** -53
    g = 2 * N * u / (1 - 2 * N * u)
    aP = np.abs(s.P)
    prior = np.diag(np.concatenate([s.cPrior, s.prior.ravel()]))
    HT = (raw["H_L"] + prior + raw["H_A"]) - raw["H_sc"]
    E0 = HLb + 3 * u * (np.abs(raw["H_L"]) + prior + np.abs(raw["H_A"]) + np.abs(raw["H_sc"]))
    Q = aP @ np.abs(HT) @ aP
    bH = (1 + lam) * ((E0 + aP @ E0 @ aP) * (1 + g) + 2 * g * Q + 2 * 3 * u * (np.abs(HT) + Q + np.abs(HM)))
    pdp = np.concatenate([s.cPrior * np.abs(s.cDelta), np.abs(s.prior * s.delta_prior).ravel()])
    bT = np.abs(raw["b_L"]) + pdp + np.abs(raw["b_A"]) + np.abs(raw["b_sc"])
    e0 = bLb + 3 * u * bT
    q = aP @ bT
    bMtop = np.abs(bM) + np.abs(HM) @ np.abs(stitched_delta(s))
    bb = (e0 + aP @ e0) * (1 + g) + 2 * g * q + 2 * 2 * u * (bT + q + bMtop) + 2 * (N + 1) * u * bMtop
    return bH, bb


def mode0_sums(T, mut=None):
    """Hdd_accAF, bd_accAF, Hcd_accAF of addPoint<0>: the residuals that are active and NOT linearized"""
    take = T.active if mut == "mode0_ignores_lin" else T.active & ~T.lin
    return lf_sums(T, T.J[:, J_RESF:J_RESF + 8], take), take


class _Fake:
    """what np_window_oracle.accumulate reads of its Oracle"""


def marginalise(T, s, rtz, pts_before, lf_before, marg, prior_fac, mut=None):
    """marginalizePointsF (EnergyFunctional.cpp:615-669) for the flagged points: priorF *= fac; addPoint<2> (resApprox = res_toZeroF,
    every active residual; the A sums zeroed); the Schur addPoint(p, false).  Returns (priorF, lf, HdiF, bdSumF, exact accumulators,
    their bound) with the unflagged points' values as they were"""
    m = np.asarray(marg) != 0
    priorF = np.where(m, T.priorF * f32(prior_fac), T.priorF).astype(f32)
    take = T.active & m[T.point]
    lf2 = lf_sums(T, rtz, take)
    lf = np.where(m[:, None], lf2, lf_before).astype(f32)
    nres = np.array([T.active[T.first[p]:T.first[p + 1]].sum() for p in range(T.n)])
    H = (f32(0) + lf[:, 0]) + priorF
    H = np.where(H < 1e-10, f32(1e-10), H).astype(f32)
    hdi = (1.0 / H.astype(np.float64)).astype(f32)
    bds = f32(0) + lf[:, 1]
    if mut == "marg_shift":
        bds = bds + priorF * T.deltaF
    live = m & (nres > 0)
    hdi, bds = np.where(live, hdi, f32(0)).astype(f32), np.where(live, bds, f32(0)).astype(f32)
    o = _Fake()
    J = T.J.copy()
    J[:, J_RESF:J_RESF + 8] = rtz
    o.r = dict(is_active=take, ef_J=J, JpJdF=T.JpJdF)
    o.p = dict(Hcd_accAF=np.zeros((T.n, 4), f32), HdiF=hdi, bdSumF=bds, nres=np.where(m, nres, 0))
    o.n, o.host, o.point, o.target, o.res_first = T.n, T.host, T.point, T.target, T.first
    acc, bound = no.accumulate(o, T.F, np.where(m[:, None], lf, f32(0)))
    return priorF, lf, hdi, bds, acc, bound


def marg_update(HM, bM, st, w, mut=None):
    """HM += w (M - Msc), bM += w (Mb - Mbsc) from the four stitched matrices"""
    if mut == "marg_sign":
        return HM + w * (st["H_A"] + st["H_sc"]), bM + w * (st["b_A"] + st["b_sc"])
    return HM + w * (st["H_A"] - st["H_sc"]), bM + w * (st["b_A"] - st["b_sc"])
