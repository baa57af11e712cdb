"""Seeded cases for the rest of setFirst (include/eds_hip_inisetup.h), built from tests/init_cases.py's frames.  A case is a first frame
and a list of makePixelStatus calls in order — (level, desired density, recursions_left, th_factor, sparsity to set first or None: what
the call before left) — so that the carried ``sparsityFactor`` is part of what is compared.

  a    a96's first frame (96 x 80, 3 levels), levels 0 .. 2 at the reference densities: level 2's desired count (1 152) exceeds its 480
       pixels, so the path runs down to sparsity 1 and the THFac = 0.5 switch.
  b    the same image quantised to multiples of 8: gradients are multiples of 4 and equal scores occur inside one cell.
  c    128 x 128, the smallest shape eds_ini_create takes for five levels, levels 1 .. 4 at the reference densities: 0.5 and 1 are
       reached on the top levels and the sparsity is carried from level to level.
  d    single passes (recursions_left = 0) on a's level 1 (48 x 40) at sparsity 1, 2, 11, 13 (the generic form) and 39 = h - 1 (no
       cells, 0 points).
  e    a constant image: nothing is above the threshold, every level has 0 points.

``expected(name)`` runs the numpy oracle once per case and is shared by the tests, which leave it unchanged."""
import functools
import types

import numpy as np

import coarse_cases as cc
import init_cases as ic
import np_init_oracle as no
import np_inisetup_oracle as nso

REFERENCE_DENSITIES = np.float32([0.03, 0.05, 0.15, 0.5, 1.0])                # CoarseInitializer.cpp:699
K128 = (110.0, 104.0, 65.3, 62.9)


def density(d, W, H):
    """CoarseInitializer.cpp:705-707: densities[lvl] * w[0] * h[0], float times int times int"""
    return np.float32(np.float32(np.float32(d) * np.float32(W)) * np.float32(H))


def _case(name, image, levels, calls):
    H, W = image.shape
    return types.SimpleNamespace(name=name, H=H, W=W, levels=levels, image=np.ascontiguousarray(image, dtype=np.float32), calls=calls,
                                 K=ic.K96 if W == 96 else K128)


@functools.lru_cache(maxsize=None)
def cases():
    a96 = ic.cases()["a96"].first
    ref = lambda l, W, H: (l, density(REFERENCE_DENSITIES[l], W, H), 5, 1.0, None)
    c = {}
    c["a"] = _case("a", a96, 3, [ref(0, 96, 80), ref(1, 96, 80), ref(2, 96, 80)])
    c["b"] = _case("b", np.round(a96 / np.float32(8)) * np.float32(8), 3, [ref(1, 96, 80), ref(2, 96, 80), ref(0, 96, 80)])
    first128 = ic.frame_at(128, 128, K128, cc.se3((0, 0, 0), (0, 0, 0)))
    c["c"] = _case("c", first128, 5, [ref(l, 128, 128) for l in range(1, 5)])
    c["d"] = _case("d", a96, 3, [(1, density(0.05, 96, 80), 0, 1.0, s) for s in (1, 2, 11, 13, 39)])
    c["e"] = _case("e", np.full((80, 96), 77.0, np.float32), 3, [ref(1, 96, 80), ref(2, 96, 80), ref(0, 96, 80)])
    return c


@functools.lru_cache(maxsize=None)
def grads(name):
    c = cases()[name]
    return no.pyramid(c.image, c.levels)


@functools.lru_cache(maxsize=None)
def expected(name):
    """per call of the case: map, n_good, passes, the sparsity left behind, the passes' trace (sparsity, THFac, numGood)"""
    c, out, sparsity = cases()[name], [], 5
    for lvl, dens, recs, th, set_first in c.calls:
        if set_first is not None:
            sparsity = set_first
        trace = []
        status, n_good, passes, sparsity = nso.make_pixel_status(grads(name)[lvl], dens, recs, th, sparsity, trace)
        status.setflags(write=False)
        out.append(types.SimpleNamespace(lvl=lvl, map=status, n_good=n_good, passes=passes, sparsity=sparsity, trace=trace))
    return out


def level_maps(name):
    """the last map the case's calls leave per level"""
    maps = {}
    for e in expected(name):
        maps[e.lvl] = e.map
    return maps
