"""Seeded cases for the window's solve (include/eds_hip_winsolve.h) on the geometry of tests/window_cases.py: the same four windows
(64 x 48; one residual with N = 20; 5 points per host; 513 points in one host, one past the 512 lanes; 1 100 + 7 x 40 points over 8 frames
with N = 68 and no residual for the pair (7, 0)), each with the state setDeltaF reads, a marginalisation prior HM / bM, a nullspace
projector formed with numpy.linalg.pinv from seven random vectors, the residuals fixLinearizationF takes and the points to marginalise,
and the rounds of solves to run.

case        linearized residuals                       rounds (iteration, lambda, mode, haveFirstFrame, projector, fac)
f2_single   its one residual                           (0, caller's 0.3, 0, yes, no, 1), (2, FIX_LAMBDA | X_LATER, yes, yes, 0.25)
f3_5        none: H_L is priors only                   (0, USE_GN | SYSTEM, yes, no, 1), (2, SYSTEM | ORTHOGONALIZE_X, NO first frame, yes, 0.25)
f3_513      every residual of every third point and    (0, FIX_LAMBDA | X_LATER, yes, yes, 1), (2, the same, 0.25)
            a tenth of the others: about a third
f8_1100     every residual of every fourth point and   (0, SYSTEM with the caller's 0.1, NO first frame, yes, 1), (2, FIX_LAMBDA | X_LATER, 0.25)
            a tenth of the others
So both assembly branches, both values of haveFirstFrame, lambda = 0 / 1e-5 / the caller's, iterations 0 and 2, with and without a
projector, fac 1 and 0.25 each followed by another linearize -> solve round occur; points without an active residual and points all of
whose residuals are linearized are in every case but f3_5.  About a tenth of the points are marginalised afterwards (in f2_single the
one point), followed by a solve with the updated HM, bM."""
import functools
import types

import numpy as np

import window_cases as wc

SVD, SYSTEM, POINTMARG, FULL, SVD_CUT7, REMOVE_POSEPRIOR, USE_GN, FIX_LAMBDA, ORTH_X, MOMENTUM, STEPMOMENTUM, X_LATER = (
    1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048)
DEFAULT = FIX_LAMBDA | X_LATER
PRIOR_FAC, WEIGHT_FAC = 2.0, 0.25


def rnd(iteration, lam, mode, hff, use_p, fac):
    return types.SimpleNamespace(iteration=iteration, lam=lam, mode=mode, hff=hff, use_p=use_p, fac=fac)


ROUNDS = {
    "f2_single": [rnd(0, 0.3, 0, True, False, 1.0), rnd(2, 7.0, DEFAULT, True, True, 0.25)],
    "f3_5": [rnd(0, 7.0, USE_GN | SYSTEM, True, False, 1.0), rnd(2, 0.0, SYSTEM | ORTH_X, False, True, 0.25)],
    "f3_513": [rnd(0, 7.0, DEFAULT, True, True, 1.0), rnd(2, 7.0, DEFAULT, True, True, 0.25)],
    "f8_1100": [rnd(0, 0.1, SYSTEM, False, True, 1.0), rnd(2, 7.0, DEFAULT, True, True, 0.25)],
}
SEEDS = {"f2_single": 101, "f3_5": 102, "f3_513": 103, "f8_1100": 104}


def extend(name, c, seed, rounds=None):
    rng = np.random.default_rng(seed)
    F, n, m = c.F, len(c.host), len(c.point)
    N = 4 + 8 * F
    s = types.SimpleNamespace(name=name, win=c, F=F, N=N, n=n, m=m, rounds=ROUNDS[name] if rounds is None else rounds)
    scale = np.array([1e-3] * 3 + [1e-3] * 3 + [1e-2, 1e-1])
    s.delta = rng.standard_normal((F, 8)) * scale
    s.delta_prior = s.delta + rng.standard_normal((F, 8)) * scale * 0.5
    s.prior = rng.uniform(1.0, 200.0, (F, 8))
    s.prior[0, :6] = 1e6                                              # the first frame's pose prior
    s.cPrior = rng.uniform(1e3, 1e5, 4)
    s.cDelta = rng.standard_normal(4) * 1e-3
    A = rng.standard_normal((N, N))
    s.HM = 3.0 * (A @ A.T) / N + np.diag(rng.uniform(1.0, 20.0, N))
    # ... and on its diagonal a tenth or so of what the window's own Hessian carries there, as a marginalisation prior has; without it
    # the scaled diagonals 1 - 10 / H_ii of two frames' translations (H_ii about 2.6e14) lie within 4 ulps of each other: a pivot tie
    typical = np.concatenate([[1e5] * 4] + [[1e14, 1e14, 1e12, 1e7, 1e7, 1e6, 1e8, 1e7]] * F)
    s.HM += np.diag(typical * rng.uniform(0.05, 0.5, N))
    s.bM = rng.standard_normal(N) * 5.0
    Nm = rng.standard_normal((N, 7))
    if any(r.mode & SYSTEM and not r.hff for r in s.rounds):
        # H -= P H P with a projector that is no nullspace of H can turn a diagonal entry negative (sqrt(diag + 10) is then NaN, in the
        # reference too).  The windows that orthogonalise the system draw the seven vectors in the metric of the Hessian's typical
        # diagonal and carry a strong marginalisation prior, so that the orthogonalised system stays solvable; the oracle checks it.
        Nm /= np.sqrt(typical)[:, None]
        s.HM += np.diag(rng.uniform(0.5e9, 2e9, N))                     # unequal, so that no two pivots tie
    Nm /= np.linalg.norm(Nm, axis=0)
    P = Nm @ np.linalg.pinv(Nm)
    s.P = 0.5 * (P + P.T)
    s.priorF, s.deltaF = c.prior, c.delta
    u = rng.random(m)
    if name == "f2_single":
        fix = np.ones(m, bool)
    elif name == "f3_5":
        fix = np.zeros(m, bool)
    elif name == "f3_513":
        fix = (c.point % 3 == 1) | (u < 0.1)
    else:
        fix = (c.point % 4 == 0) | (u < 0.1)
    s.fix = fix.astype(np.int32)
    marg = rng.random(n) < 0.1
    if n == 1:
        marg[:] = True
    s.marg = marg.astype(np.int32)
    s.fix_marg = marg[c.point].astype(np.int32) if m else np.zeros(0, np.int32)       # fixed before the marginalisation: every residual of a flagged point
    return s


@functools.lru_cache(maxsize=None)
def cases():
    return {k: extend(k, c, SEEDS[k]) for k, c in wc.cases().items()}
