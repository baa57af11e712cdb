"""What the tests of include/eds_hip_winedit.h edit: the windows of tests/winsolve_cases.py, one larger window whose points and residuals
each span several workgroups of the scan (1 024 rows) and of the gathers, and the flag patterns — each a list of steps
("points", flag) / ("residuals", select or None) run one after the other on one prepared window.

pattern        steps
none           no point flagged; no residual selected
all            every residual selected; then every point flagged (their runs are empty by then)
first_last     the first and the last point; then the first and the last residual
host0          every point of the first host that has points: its run becomes empty
host_last      every point of the last host that has points
empty_run      every residual of the first, a middle and the last point, so that those points keep an EMPTY run; then every fourth point
               (a point with an empty run among the flagged and among the kept); then the points with empty runs
null_select    select == NULL: every residual whose state is not IN (the states hold OOB and OUTLIER after an apply)
random30       a random 30 % of the points (flags are arbitrary nonzero words); then a random 30 % of the residuals
marginalised   the case's marg flags, after eds_wsv_marginalize_points with the same array (the tests run that first)
"""
import copy
import functools
import types

import numpy as np

import window_cases as wc
import winsolve_cases as wsc

PATTERNS = ("none", "all", "first_last", "host0", "host_last", "empty_run", "null_select", "random30", "marginalised")
BIG = "f8_4500"


@functools.lru_cache(maxsize=None)
def cases():
    """the four windows of winsolve_cases and f8_4500: 1 500 + 7 x 430 points over 8 frames, about 20 000 residuals"""
    out = dict(wsc.cases())
    c = wc.make(5, 8, [1500] + [430] * 7, shift=1, targets_per_point=4)
    out[BIG] = wsc.extend(BIG, c, 105, rounds=wsc.ROUNDS["f3_513"])
    return out


def steps(pattern, s, n, m, host, point, seed=7):
    """the steps of `pattern` for a window that holds n points (hosts `host`) and m residuals (points `point`) before the first step.
    A later step's flags are sized for what the earlier steps leave, which this function works out from the flags alone."""
    rng = np.random.default_rng(seed + n + 31 * m)
    zp, zr = np.zeros(n, np.int32), np.zeros(m, np.int32)
    if pattern == "none":
        return [("points", zp), ("residuals", zr)]
    if pattern == "all":
        return [("residuals", zr + 1), ("points", zp + 1)]
    if pattern == "first_last":
        f = zp.copy()
        f[[0, n - 1]] = 1
        m2 = int((f[point] == 0).sum())
        r = np.zeros(m2, np.int32)
        if m2:
            r[[0, m2 - 1]] = 1
        return [("points", f), ("residuals", r)]
    if pattern in ("host0", "host_last"):
        h = host[0] if pattern == "host0" else host[-1]
        return [("points", (host == h).astype(np.int32))]
    if pattern == "empty_run":
        chosen = sorted({0, n // 2, n - 1})
        sel = np.isin(point, chosen).astype(np.int32)
        f = (np.arange(n) % 4 == 0).astype(np.int32)                      # point 0 (empty run) goes, n // 2 or n - 1 may stay
        kept = np.flatnonzero(f == 0)
        f2 = np.isin(kept, chosen).astype(np.int32)
        return [("residuals", sel), ("points", f), ("points", f2)]
    if pattern == "null_select":
        return [("residuals", None)]
    if pattern == "random30":
        f = np.where(rng.random(n) < 0.3, rng.integers(1, 2 ** 31 - 1, n), 0).astype(np.int32)
        f[f != 0] *= rng.choice([-1, 1], int((f != 0).sum())).astype(np.int32)
        m2 = int((f[point] == 0).sum())
        r = (rng.random(m2) < 0.3).astype(np.int32) * np.int32(-2 ** 31)
        return [("points", f), ("residuals", r.astype(np.int32))]
    if pattern == "marginalised":
        return [("points", s.marg.astype(np.int32))]
    raise KeyError(pattern)


def frames_of(F):
    """the frames a test marginalises: the first, a middle one and the last (which takes no permutation branch)"""
    return sorted({0, F // 2, F - 1})


def reduce_case(s, frame):
    """case s as the caller sees it once `frame` has left: F - 1 frames, every per-frame and per-pair input without that frame, one
    round without a projector.  HM / bM are the caller's to fill in from eds_wed_marginalize_frame."""
    c, F = s.win, s.F
    keep = [f for f in range(F) if f != frame]
    pair = lambda a, tail: np.asarray(a).reshape((F, F) + tail)[np.ix_(keep, keep)].reshape((-1,) + tail)      # noqa: E731
    win = copy.copy(c)
    win.F = F - 1
    win.images, win.th = c.images[keep], c.th[keep]
    win.precalc = pair(c.precalc, (27,))                         # [h F + t]
    win.adH, win.adT = pair(c.adH, (8, 8)), pair(c.adT, (8, 8))  # [h + F t]: the same two axes, the other way round
    out = types.SimpleNamespace(name=f"{s.name}-{frame}", win=win, F=F - 1, N=s.N - 8, delta=s.delta[keep], prior=s.prior[keep],
                                delta_prior=s.delta_prior[keep], cPrior=s.cPrior, cDelta=s.cDelta, HM=None, bM=None, P=None,
                                rounds=[wsc.rnd(0, 0.0, wsc.DEFAULT, True, False, 1.0)])
    return out


# ---- activated points enter: windows over the frames of tests/activate_cases.py ------------------------------------------------------------

INSERT_NAMES = ("w64_f3", "w64_f3_frac", "w64_f2_noactive", "m96_f8_obs3")      # F = 3, 3, 2 (nothing is activated), 8 (host 2 has no point)


def tables_of(activated, F):
    """Activation.window_tables() from the arrays of eds_act_get_activated (or of np_activate_oracle.activated)"""
    a = activated
    pt = [i for i, mask in enumerate(a["target_mask"]) for t in range(F) if (int(mask) >> t) & 1]
    tg = [t for mask in a["target_mask"] for t in range(F) if (int(mask) >> t) & 1]
    m = len(pt)
    points = dict(host=a["host"], uv=a["uv"], color=a["color"], weights=a["weights"], idepth_scaled=a["idepth"], idepth_zero_scaled=a["idepth"])
    residuals = dict(point=np.array(pt, np.int32), target=np.array(tg, np.int32), state=np.zeros(m, np.int32), energy=np.zeros(m, np.float32))
    return points, residuals


@functools.lru_cache(maxsize=None)
def insert_case(name, per_host=6, seed=9):
    """a window over the frames of activate case `name` that already holds per_host points in every host but the last-but-one (an empty
    run in the middle of the merge), each observed in every other frame, and the state the edits carry along"""
    import activate_cases as ac
    return _insert_case_of(ac.cases()[name], per_host, seed)


@functools.lru_cache(maxsize=None)
def cycle_case():
    """F = 4, 96 x 128: the window and the eds_imm of the keyframe-cycle test (an activation case of its own, made as those of
    tests/activate_cases.py are), with the marginalisation prior the cycle carries"""
    import activate_cases as ac
    c = ac.make_case("c128_f4", 71, 96, 128, (110.0, 104.0, 66.5, 45.25), [40, 30, 30, 24], 0.03, (0.02, 0.005, 0.002), 20, dict(), 2.0)
    s = _insert_case_of(c, 6, 9, empty_host=False)
    rng = np.random.default_rng(72)
    A = rng.standard_normal((s.N, s.N))
    s.HM = A @ A.T / s.N + np.diag(rng.uniform(1e3, 1e4, s.N))
    s.bM = rng.standard_normal(s.N)
    s.rounds = [wsc.rnd(0, 0.0, wsc.DEFAULT, True, False, 1.0)]
    s.P = None
    return s


def _insert_case_of(c, per_host, seed, empty_host=True):
    import activate_cases as ac
    import immature_cases as ic
    name = c.name
    F = c.F
    rng = np.random.default_rng(seed + F)
    host = np.array([h for h in range(F) for _ in range(per_host) if not empty_host or h != F - 2 or F == 2], np.int32)
    n = len(host)
    point = np.repeat(np.arange(n, dtype=np.int32), F - 1)
    target = np.array([t for h in host for t in range(F) if t != h], np.int32)
    pre27 = np.zeros((F, F, 27), np.float32)
    for i in range(F):
        for t in range(F):
            R, tr = ac.relative(c.poses, i, t)
            KRKi, Kt, _ = ic.precalc32(c.K4, R, tr)
            pre27[i, t] = np.concatenate([KRKi.ravel(), Kt, c.pre[i, t, :12], c.pre[i, t, 12:], [0.0]])
    win = types.SimpleNamespace(H=c.H, W=c.W, F=F, K=tuple(c.K4), prm={}, images=np.stack(c.images).astype(np.float32), host=host,
                                uv=np.stack([rng.integers(8, c.W - 8, n), rng.integers(8, c.H - 8, n)], axis=1).astype(np.float32),
                                color=rng.uniform(40, 200, (n, 8)).astype(np.float32), weights=rng.uniform(0.5, 1.0, (n, 8)).astype(np.float32),
                                ids=rng.uniform(0.3, 0.8, n).astype(np.float32), point=point, target=target, state=np.zeros(len(point), np.int32),
                                energy=rng.uniform(0, 50, len(point)).astype(np.float32), precalc=pre27.reshape(-1, 27),
                                th=np.full(F, 12 * 12 * 8, np.float32), adH=np.tile(np.eye(8), (F * F, 1, 1)), adT=np.tile(-np.eye(8), (F * F, 1, 1)))
    win.idz = (win.ids * np.float32(1.01)).astype(np.float32)
    return types.SimpleNamespace(name=name, act=c, win=win, F=F, N=4 + 8 * F, delta=rng.standard_normal((F, 8)) * 1e-3, prior=np.ones((F, 8)),
                                 delta_prior=np.zeros((F, 8)), cPrior=np.ones(4), cDelta=np.zeros(4), priorF=rng.uniform(0, 5, n).astype(np.float32),
                                 deltaF=(win.ids - win.idz).astype(np.float32), fix=(np.arange(len(point)) % 2).astype(np.int32))


def prepare_insert(w, sv, s):
    """linearize -> apply -> set_state -> fix_linearization -> backup: rows of every kind hold something before the insert"""
    c = s.win
    w.linearize(c.F, c.precalc, c.th)
    w.apply(True)
    sv.set_state(s.F, c.adH, c.adT, s.delta, s.prior, s.delta_prior, s.cPrior, s.cDelta, s.priorF, s.deltaF)
    sv.fix_linearization(s.fix)
    sv.backup_idepths()
