"""Pins makeNN's neighbour and parent tables (CoarseInitializer.cpp:884-958) to the reference's own nanoflann, ties included.

tests/golden/nn/ref_nn_*.npz hold what src/utils/nanoflann.h — compiled unmodified by oracle/ref/Makefile into oracle/_ref/nanoflann_nn and
called as makeNN calls it — returned for levels of 1 .. 257 lattice points, a third of a 40 x 32 level, a full rectangle, a row, a
column, a window at x = 8 000, levels above of 700 points, of one point and off to one side, identical and duplicated points,
real-valued clouds, a tree deeper than the explicit walk's stack, and near-ties an FMA would decide the other way.  Against them, always:
  * the oracle (tests/np_nn_oracle.py: nanoflann's build and walk in plain Python with np.float32 scalars);
  * the product's host build and both of its walks (slam-eds_amd/csrc/eds_nntree.hpp under g++ through tests/host_logic/inisetup_harness.cpp).
Where oracle/_ref/nanoflann_nn exists, a seeded fuzz compares both with nanoflann live.  On a GPU, every lattice golden goes through
eds_ini_set_points and eds_ini_make_neighbours and must come back as the reference's table."""
import importlib
import os
import sys

import numpy as np
import pytest

import inisetup_harness as sh
import nn_cases as nc
import np_nn_oracle as nno

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle", "ref"))
import refcase  # noqa: E402

NAMES = nc.golden_names()
LATTICE = nc.lattice_names()
THIRD = "ref_nn_lattice_40x32_third.npz"
THIRD_ROWS, THIRD_SETS, THIRD_N = 211, 53, 260        # what tests/golden/make_ref_nn_golden.py printed for it
KEYS = (("nb", "ref_nb"), ("dist", "ref_dist"), ("parent", "ref_parent"), ("parent_dist", "ref_parent_dist"))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _assert_equals_golden(got, g, what):
    for k, gk in KEYS:
        assert got[k].shape == g[gk].shape, (what, k)
        bad = np.argwhere(_bits(got[k]) != _bits(g[gk]))
        assert len(bad) == 0, f"{what}: {k} differs in {len(bad)} places, first at {bad[:4].tolist()}"


def test_goldens_are_there():
    assert len(NAMES) == 25 and len(LATTICE) == 19, NAMES
    for n in (1, 2, 5, 6, 9, 10, 11, 12, 63, 65, 257):
        g = nc.load(f"ref_nn_count_{n:03d}.npz")
        assert len(g["uv"]) == n and ((g["ref_nb"] >= 0).sum(axis=1) == min(n, 10)).all() and (g["ref_parent"] >= 0).all()
    assert len(nc.load("ref_nn_parents_700.npz")["uv_up"]) == 700 and len(nc.load("ref_nn_parents_1.npz")["uv_up"]) == 1
    assert len(nc.load("ref_nn_lattice_full_33x25.npz")["uv"]) == 33 * 25
    g = nc.load("ref_nn_lattice_x8000.npz")                                        # fp32 steps of 2^-11: u's fraction is 205 / 2048, not v's
    frac = g["uv"].astype(np.float64) % 1
    assert g["uv"][:, 0].min() > 8000 and (frac[:, 0] == 205 / 2048).all() and (np.abs(frac[:, 1] - 0.1) < 1e-6).all()
    g = nc.load("ref_nn_parents_outside_hull.npz")
    q = g["uv"] * np.float32(0.5) - np.float32(0.25)
    assert (q[:, 0] > g["uv_up"][:, 0].max()).mean() > 0.5
    for name in LATTICE:                                                           # lattice cases are levels: status maps give them back
        g = nc.load(name)
        H, W = int(g["H"]), int(g["W"])
        assert np.array_equal(nc.lattice_uv(nc.status_from_uv(g["uv"], H, W)), g["uv"]), name
        assert np.array_equal(nc.lattice_uv(nc.status_from_uv(g["uv_up"], H // 2, W // 2)), g["uv_up"]), name


def test_goldens_discriminate_the_exhaustive_lower_index_rule():
    """the rule the product had — ten smallest fp32 squared distances, ties to the lower index — gives other rows, and other SETS of
    neighbours, on a third of a 40 x 32 level: the counts the generator found"""
    g = nc.load(THIRD)
    ex, _ = sh.make_nn_exhaustive(g["uv"], g["uv_up"])
    assert np.array_equal(ex, nno.exhaustive(g["uv"]))
    assert len(g["uv"]) == THIRD_N
    assert int((ex != g["ref_nb"]).any(axis=1).sum()) == THIRD_ROWS
    assert int((np.sort(ex, axis=1) != np.sort(g["ref_nb"], axis=1)).any(axis=1).sum()) == THIRD_SETS
    # the distances agree as multisets: only ties are decided differently
    d = lambda nb: np.sort(((g["uv"][:, None, :] - g["uv"][nb]) ** 2).sum(-1), axis=1)
    assert np.array_equal(d(ex), d(g["ref_nb"]))


def test_near_tie_golden_needs_separate_rounding():
    """at every site the reference's second neighbour (the first is the point itself) and the reference's parent are not what a search
    with d0 d0 + d1 d1 contracted into an FMA prefers"""
    g = nc.load("ref_nn_near_tie_fma.npz")
    uv, up = g["uv"], g["uv_up"]
    sites = len(uv) // 3
    assert sites == 48 and len(up) == 2 * sites
    for k in range(sites):
        q = uv[3 * k]
        assert g["ref_nb"][3 * k, 0] == 3 * k and sorted(g["ref_nb"][3 * k, 1:3]) == [3 * k + 1, 3 * k + 2]
        assert nc.contracted_winner(uv, q, [3 * k + 1, 3 * k + 2], k % 2) != g["ref_nb"][3 * k, 1], k
        p = (q[0] * np.float32(0.5) - np.float32(0.25), q[1] * np.float32(0.5) - np.float32(0.25))
        assert g["ref_parent"][3 * k] in (2 * k, 2 * k + 1)
        assert nc.contracted_winner(up, p, [2 * k, 2 * k + 1], (k + 1) % 2) != g["ref_parent"][3 * k], k


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_reference_nanoflann(name):
    g = nc.load(name)
    _assert_equals_golden(nno.make_nn(g["uv"], g["uv_up"]), g, name)


@pytest.mark.parametrize("name", NAMES)
def test_product_host_equals_reference_nanoflann(name):
    """both walks: the explicit stack (where the tree fits it) and the recursion that takes deeper trees"""
    g = nc.load(name)
    got = sh.make_nn(g["uv"], g["uv_up"])
    _assert_equals_golden(got, g, name)
    _assert_equals_golden(sh.make_nn(g["uv"], g["uv_up"], stack=0), g, name + " (recursive walk)")
    o = nno.make_nn(g["uv"], g["uv_up"])
    assert (got["depth"], got["depth_up"]) == (o["depth"], o["depth_up"])
    if name in LATTICE:
        assert max(got["depth"], got["depth_up"]) <= sh.nn_stack()          # levels never need the recursion


def test_a_tree_deeper_than_the_stack_takes_the_recursive_walk():
    g = nc.load("ref_nn_deep_tree.npz")
    got = sh.make_nn(g["uv"], g["uv_up"])
    assert got["depth"] > sh.nn_stack() == 64 and got["depth_up"] <= sh.nn_stack()
    _assert_equals_golden(got, g, "deep tree")
    # a shallower stack limit sends more trees to the recursion, with the same tables
    h = nc.load(THIRD)
    want = sh.make_nn(h["uv"], h["uv_up"])
    assert 1 < want["depth"] < 20
    for stack in (want["depth"] - 1, want["depth"], 1):
        _assert_equals_golden(sh.make_nn(h["uv"], h["uv_up"], stack=stack), h, f"stack {stack}")


def test_top_level_has_no_parents():
    g = nc.load(THIRD)
    got = sh.make_nn(g["uv"], None)
    assert np.array_equal(got["nb"], g["ref_nb"]) and (got["parent"] == -1).all()
    assert np.array_equal(nno.make_nn(g["uv"], None)["nb"], g["ref_nb"])


def _fuzz_case(rng, t):
    kind = t % 6
    if kind == 0:                                   # a level with holes
        H, W = rng.integers(9, 48, 2)
        uv = nc.lattice_uv(rng.random((H, W)) >= rng.uniform(0, 0.6))
    elif kind == 1:                                 # every other / every third pixel
        H, W = rng.integers(10, 60, 2)
        m = np.zeros((H, W), dtype=bool)
        step = int(rng.integers(2, 4))
        m[::step, ::step] = True
        uv = nc.lattice_uv(m & (rng.random((H, W)) >= rng.uniform(0, 0.4)))
    elif kind == 2:                                 # duplicates
        H, W = rng.integers(9, 30, 2)
        b = nc.lattice_uv(rng.random((H, W)) >= 0.3)
        uv = np.concatenate([b, b[rng.integers(0, max(1, len(b)), len(b))]]) if len(b) else b
        uv = uv[rng.permutation(len(uv))]
    elif kind == 3:                                 # tiny n
        uv = (rng.integers(0, 6, (int(rng.integers(1, 14)), 2)) + 0.1).astype(np.float32)
    elif kind == 4:                                 # real-valued
        uv = (rng.normal(0, 1, (int(rng.integers(1, 300)), 2)) * rng.choice([1e-3, 1.0, 100.0])).astype(np.float32)
    else:                                           # integer cloud, heavy ties
        H, W = rng.integers(4, 40, 2)
        uv = rng.integers(0, [W, H], (int(rng.integers(1, 400)), 2)).astype(np.float32)
    if len(uv) == 0:
        uv = np.array([[3.1, 3.1]], np.float32)
    # the level above: a lattice at half the size, a real-valued cloud, one point, or none
    pk = int(rng.integers(0, 4))
    lo, hi = uv.min(axis=0) * 0.5 - 2, uv.max(axis=0) * 0.5 + 2
    if pk == 0:
        up = (rng.integers(np.floor(lo), np.ceil(hi) + 1, (int(rng.integers(1, 200)), 2)) + 0.1).astype(np.float32)
    elif pk == 1:
        up = rng.uniform(lo, hi, (int(rng.integers(1, 100)), 2)).astype(np.float32)
    elif pk == 2:
        up = rng.uniform(lo - 50, hi + 50, (1, 2)).astype(np.float32)
    else:
        up = None
    return uv, up


def test_fuzz_oracle_and_product_equal_reference_nanoflann():
    if not refcase.nanoflann_available():
        pytest.skip("oracle/_ref/nanoflann_nn is not built here (no reference tree): the golden cases above still pin makeNN")
    rng = np.random.default_rng(11)
    for t in range(600):
        uv, up = _fuzz_case(rng, t)
        r = refcase.nanoflann_nn(uv, up)
        g = dict(ref_nb=r["nb"], ref_dist=r["dist"], ref_parent=r["parent"], ref_parent_dist=r["parent_dist"])
        _assert_equals_golden(sh.make_nn(uv, up, stack=None if t % 3 else 0), g, f"product host, case {t} (n = {len(uv)})")
        _assert_equals_golden(nno.make_nn(uv, up), g, f"oracle, case {t} (n = {len(uv)})")


# ---- the device -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", LATTICE)
def test_device_tables_equal_reference_nanoflann(gpu, name):
    """the golden's level and the level above as status maps through eds_ini_set_points, then eds_ini_make_neighbours: the points are
    the golden's bit for bit and the tables are the reference's.  Reads tests/golden/nn/ only."""
    init = importlib.import_module("slam-eds_amd.init")
    g = nc.load(name)
    H, W = int(g["H"]), int(g["W"])
    with init.CoarseInitializer(H, W, 2, max_points_per_level=1024) as t:
        assert t.set_points(0, nc.status_from_uv(g["uv"], H, W)) == len(g["uv"])
        assert t.set_points(1, nc.status_from_uv(g["uv_up"], H // 2, W // 2)) == len(g["uv_up"])
        for l, want in ((0, g["uv"]), (1, g["uv_up"])):
            p = t.points(l)
            assert np.array_equal(_bits(np.stack([p["u"], p["v"]], axis=1)), _bits(want)), (name, l)
        t.make_neighbours()
        nb, par = t.neighbours(0)
        bad = np.argwhere(nb != g["ref_nb"])
        assert len(bad) == 0, f"{name}: {len(np.unique(bad[:, 0]))} of {len(nb)} rows differ, first at {bad[:4].tolist()}"
        assert np.array_equal(par, g["ref_parent"]), f"{name}: {(par != g['ref_parent']).sum()} parents differ"
        nb_up, par_up = t.neighbours(1)                                            # the top level: the pinned host walk's table
        assert par_up is None and np.array_equal(nb_up, sh.make_nn(g["uv_up"])["nb"])
        if name == THIRD:                                                          # ... and no longer the exhaustive lower-index rule's
            ex, _ = sh.make_nn_exhaustive(g["uv"], g["uv_up"])
            assert int((nb != ex).any(axis=1).sum()) == THIRD_ROWS
            assert int((np.sort(nb, axis=1) != np.sort(ex, axis=1)).any(axis=1).sum()) == THIRD_SETS
