"""Point levels for CoarseInitializer::makeNN (CoarseInitializer.cpp:884-958) — test helpers.

The reference finds every point's ten neighbours and its parent with nanoflann (src/utils/nanoflann.h); equal distances are decided
by the order its tree is visited in.  Real levels tie all the time: setFirst (:718-749) puts a point at (float)(x + 0.1), (float)(y + 0.1)
for selected integer pixels of the rectangle 3 <= x < w - 4, 3 <= y < h - 4, in row-major order.  The helpers here build such levels,
and real-valued clouds with constructed near-ties whose winner depends on how d0 d0 + d1 d1 is rounded.

Golden files (tests/golden/nn/ref_nn_*.npz, written by tests/golden/make_ref_nn_golden.py from the reference's own nanoflann) hold
    uv, uv_up                  float32 n x 2, n_up x 2 (n_up = 0: no level above)
    ref_nb, ref_dist           int32 / float32 n x 10: the ten neighbours in nanoflann's order and their squared distances (-1 / 0 where
                               the level has fewer than ten points)
    ref_parent, ref_parent_dist  int32 / float32 n: the nearest point of uv_up to 0.5f pt - 0.25f (-1 / 0 without a level above)
    H, W                       lattice cases only: the size of the level uv lies in (level 0 of a handle; uv_up lies in H/2 x W/2)
"""
import glob
import os
from fractions import Fraction

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nn")
F = np.float32


def rect_mask(h, w):
    """setFirst's rectangle (:722) as a mask of the h x w level"""
    m = np.zeros((h, w), dtype=bool)
    m[3:h - 4, 3:w - 4] = True
    return m


def lattice_uv(mask):
    """the level's points for a status mask: the rectangle in row-major order, u = (float)(x + 0.1) (:727-728)"""
    mask = np.asarray(mask, dtype=bool)
    ys, xs = np.nonzero(mask & rect_mask(*mask.shape))
    return np.stack([(xs + 0.1).astype(np.float32), (ys + 0.1).astype(np.float32)], axis=1)


def status_from_uv(uv, h, w):
    """the float status map eds_ini_set_points takes, from lattice points"""
    s = np.zeros((h, w), np.float32)
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    xs, ys = np.rint(uv[:, 0] - 0.1).astype(int), np.rint(uv[:, 1] - 0.1).astype(int)
    s[ys, xs] = 1
    assert s.sum() == len(uv) and not (s.astype(bool) & ~rect_mask(h, w)).any()
    return s


def pick_mask(rng, h, w, k, x0=None, x1=None):
    """exactly k pixels of setFirst's rectangle (columns x0 <= x < x1 of it, if given)"""
    ok = rect_mask(h, w)
    if x0 is not None:
        ok[:, :x0] = False
        ok[:, x1:] = False
    ys, xs = np.nonzero(ok)
    pick = rng.choice(len(ys), size=k, replace=False)
    m = np.zeros((h, w), dtype=bool)
    m[ys[pick], xs[pick]] = True
    return m


def load(name):
    g = np.load(os.path.join(GOLDEN, name))
    return {k: g[k] for k in g.files}


def golden_names():
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "ref_nn_*.npz")))


def lattice_names():
    return [n for n in golden_names() if "H" in np.load(os.path.join(GOLDEN, n)).files]


# ---- near ties ---------------------------------------------------------------------------------------------------------------------
def round_f32(x):
    """a Fraction to the nearest float32 (ties cannot be told apart here and are refused)"""
    f = F(float(x))
    cands = [np.nextafter(f, F(-np.inf)), f, np.nextafter(f, F(np.inf))]
    err = [abs(Fraction(float(c)) - x) for c in cands]
    best = int(np.argmin(err))
    if sorted(err)[0] == sorted(err)[1]:
        raise ArithmeticError("a tie in rounding")
    return cands[best]


def d2_separate(q, t):
    """FLANNPointcloud::kdtree_distance: every difference, product and sum rounded to fp32 on its own"""
    d0, d1 = F(q[0]) - F(t[0]), F(q[1]) - F(t[1])
    return d0 * d0 + d1 * d1


def d2_contracted(q, t, form):
    """d0 d0 + d1 d1 with one product folded into an FMA: form 0 is fma(d0, d0, d1 d1), form 1 is fma(d1, d1, d0 d0)"""
    d0, d1 = F(q[0]) - F(t[0]), F(q[1]) - F(t[1])
    if form == 1:
        d0, d1 = d1, d0
    return round_f32(Fraction(float(d0)) * Fraction(float(d0)) + Fraction(float(d1 * d1)))


def near_tie_pair(rng, q, form, radius=(0.4, 1.0), tries=200000):
    """Two fp32 points about q whose order in squared distance is strict with separate rounding and reversed under the contracted form"""
    q = np.asarray(q, dtype=np.float32)
    for _ in range(tries):
        r, th = rng.uniform(*radius), rng.uniform(0, 2 * np.pi)
        a = (q.astype(np.float64) + [r * np.cos(th), r * np.sin(th)]).astype(np.float32)
        sa = float(d2_separate(q, a))
        x = float(q[0]) + rng.uniform(-1, 1) * np.sqrt(sa) * 0.9
        b = np.array([x, float(q[1]) + np.sqrt(max(sa - (float(q[0]) - x) ** 2, 0.0)) * rng.choice([-1.0, 1.0])]).astype(np.float32)
        sa, sb = d2_separate(q, a), d2_separate(q, b)
        if sa == sb:
            continue
        try:
            ca, cb = d2_contracted(q, a, form), d2_contracted(q, b, form)
        except ArithmeticError:
            continue
        if ca != cb and (ca < cb) != (sa < sb):
            return a, b
    raise RuntimeError(f"no near-tie about {q} in {tries} tries")


def near_tie_sites(rng, nx, ny, spacing=8.0):
    """nx x ny sites `spacing` apart.  Level: the site's point q and a near-tie pair about it, rows 3k, 3k + 1, 3k + 2 (the pair in random
    order), reversed under contracted form k % 2; the level above: a near-tie pair about 0.5f q - 0.25f, rows 2k, 2k + 1, reversed under
    form (k + 1) % 2.  Returns (uv, uv_up)."""
    uv, up = [], []
    for j in range(ny):
        for i in range(nx):
            q = np.array([5.0 + spacing * i + rng.uniform(0, 1), 5.0 + spacing * j + rng.uniform(0, 1)]).astype(np.float32)
            k = j * nx + i
            a, b = near_tie_pair(rng, q, k % 2)
            uv.extend([q, a, b] if rng.random() < 0.5 else [q, b, a])
            p = np.array([q[0] * F(0.5) - F(0.25), q[1] * F(0.5) - F(0.25)], dtype=np.float32)
            a, b = near_tie_pair(rng, p, (k + 1) % 2, radius=(0.3, 0.8))
            up.extend([a, b] if rng.random() < 0.5 else [b, a])
    return np.asarray(uv, dtype=np.float32), np.asarray(up, dtype=np.float32)


def contracted_winner(points, q, cand, form):
    """among the candidate rows of `points`, the one a search with a contracted distance would prefer (strictly nearer)"""
    d = [d2_contracted(q, points[i], form) for i in cand]
    return cand[int(np.argmin(d))]
