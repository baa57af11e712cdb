"""What the tests of include/eds_hip_winflag.h run on: the windows of tests/winsolve_cases.py (F = 3 and F = 8) and the large window of
tests/winedit_cases.py (4 510 points: more than one tile of the scan), each with a hand-made history in which lastResiduals names a
residual the point has, one it does not have, nothing, or the same target twice, and max_rel_baseline lies below and above what the
residuals give."""
import functools
import types

import numpy as np

import winedit_cases as wec

NAMES = ("f3_5", "f3_513", "f8_1100", wec.BIG)
SEEDS = dict(zip(NAMES, (41, 42, 43, 44)))


def history_for(host, point, target, F, seed):
    """a history for the tables given: every kind of lastResiduals entry, counts 0 .. 20, maxima 0 and up to 2 (relBS is 0.01 times a
    displacement in pixels), is_new on about half of the residuals (any nonzero word is a flag)"""
    rng = np.random.default_rng(seed)
    n, m = len(host), len(point)
    first = np.searchsorted(point, np.arange(n + 1))
    lt = np.full((n, 2), -1, np.int32)
    for p in range(n):
        own = list(target[first[p]:first[p + 1]])
        other = [f for f in range(F) if f not in own]
        for k in range(2):
            kind = rng.integers(0, 4)
            if kind == 0 and own:
                lt[p, k] = rng.choice(own)
            elif kind == 1 and other:
                lt[p, k] = rng.choice(other)
            elif kind == 2 and k == 1:
                lt[p, 1] = lt[p, 0]                              # both entries name one residual: only [0] follows it
    is_new = np.where(rng.random(m) < 0.5, rng.integers(1, 2 ** 31 - 1, m) * rng.choice([-1, 1], m), 0).astype(np.int32)
    return dict(num_good=rng.integers(0, 21, n).astype(np.int32),
                max_rel_baseline=np.where(rng.random(n) < 0.4, 0.0, rng.uniform(0.0, 2.0, n)).astype(np.float32),
                last_target=lt, last_state=rng.integers(0, 3, (n, 2)).astype(np.int32), is_new=is_new)


@functools.lru_cache(maxsize=None)
def case(name):
    """the solver case, its tables as plain arrays, made-up states and active marks for the tests without a window, and the history"""
    s = wec.cases()[name]
    c = s.win
    rng = np.random.default_rng(SEEDS[name] + 100)
    m = len(c.point)
    state = rng.choice([0, 0, 0, 1, 2], m).astype(np.int32)
    active = ((state == 0) & (rng.random(m) < 0.8)).astype(np.int32)
    return types.SimpleNamespace(name=name, s=s, F=c.F, host=c.host, uv=c.uv, ids=c.ids, point=c.point, target=c.target, precalc=c.precalc, state=state,
                                 active=active, history=history_for(c.host, c.point, c.target, c.F, SEEDS[name]))


@functools.lru_cache(maxsize=None)
def flag_case(F, n, seed):
    """hand-made tables for the flagging decision alone: runs of 0 .. F - 1 residuals, and every value a comparison of isOOB,
    isInlierNew or the Hessian threshold turns on, at it and on either side of it"""
    rng = np.random.default_rng(seed)
    host = np.sort(rng.integers(0, F, n)).astype(np.int32)
    point, target = [], []
    for p in range(n):
        size = int(rng.choice([0, 1, 2, 3, 3, 4, F - 1]))
        others = [t for t in range(F) if t != host[p]]
        ts = sorted(rng.choice(others, min(size, len(others)), replace=False).tolist())
        point += [p] * len(ts)
        target += ts
    point, target = np.array(point, np.int32).reshape(-1), np.array(target, np.int32).reshape(-1)
    m = len(point)
    hist = history_for(host, point, target, F, seed + 1)
    hist["num_good"] = rng.choice([0, 3, 4, 5, 13, 14, 15, 16, 20], n).astype(np.int32)
    return types.SimpleNamespace(F=F, host=host, point=point, target=target, history=hist, state=rng.choice([0, 0, 0, 1, 2], m).astype(np.int32),
                                 ids=rng.choice([-1.0, -0.0, 0.0, 0.5, 0.5, 0.5, 1.5], n).astype(np.float32),
                                 hessian=rng.choice([0.0, 49.99, 50.0, 50.01, 1000.0], n).astype(np.float32),
                                 masks=[0, 1, 1 << (F - 1), 5 % (1 << F), (1 << F) - 1])


FLAG_CASES = ((3, 60, 1), (8, 400, 2), (8, 4510, 3))


def keep_patterns(m, seed):
    """which residuals stay: all, none, every third leaves, a random 30 % leaves"""
    rng = np.random.default_rng(seed)
    return dict(all=np.ones(m, np.int32), none=np.zeros(m, np.int32), third=(np.arange(m) % 3 != 0).astype(np.int32), random=(rng.random(m) >= 0.3).astype(np.int32))
