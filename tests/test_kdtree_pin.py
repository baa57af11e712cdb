"""Pins the keyframe's depth association (KeyFrame.cpp:1137-1166) to the reference's own k-d tree, ties included.

tests/golden/kdtree/ref_kdtree_*.npz hold the index and minDist that src/utils/KDTree.hpp — compiled unmodified by oracle/ref/Makefile into
oracle/_ref/kdtree_nn — returned for every query of pixel grids with holes, duplicates, a single row / column, m = 1..4, queries on
split planes and outside the hull, and real-valued near-ties.  Against them, always:
  * the oracle (pyoracle.kdtree_nn, behind np_keyframe_oracle.set_depth_map);
  * the product's host build plus its walk (slam-eds_amd/csrc/eds_kdtree.hpp, compiled with g++ through tests/host_logic/harness.cpp).
Where oracle/_ref/kdtree_nn exists, a seeded fuzz compares both with the reference tree live."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import kdtree_cases as kc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle", "ref"))
import refcase  # noqa: E402

SRC = os.path.join(HERE, "host_logic", "harness.cpp")
LIB = os.path.join(HERE, "host_logic", "libhost_logic.so")
_dp = C.POINTER(C.c_double)
NAMES = kc.golden_names()


@pytest.fixture(scope="module")
def hl():
    deps = [SRC] + [os.path.join(ROOT, p) for p in ("oracle/eds_oracle.hpp", "slam-eds_amd/csrc/eds_math.hpp", "slam-eds_amd/csrc/eds_solver.hpp",
                                                   "slam-eds_amd/csrc/eds_layout.hpp", "slam-eds_amd/csrc/eds_launch_rule.hpp",
                                                   "slam-eds_amd/csrc/eds_kdtree.hpp")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-misleading-indentation", "-o", LIB, SRC])
    return C.CDLL(LIB)


def host_walk(hl, xy, q):
    xy, q = np.ascontiguousarray(xy, dtype=np.float64), np.ascontiguousarray(q, dtype=np.float64)
    idx, dist = np.zeros(len(q), dtype=np.int32), np.zeros(len(q))
    hl.hl_kdtree_nn(xy.ctypes.data_as(_dp), C.c_int(len(xy)), q.ctypes.data_as(_dp), C.c_int(len(q)), idx.ctypes.data_as(C.POINTER(C.c_int32)),
                    dist.ctypes.data_as(_dp))
    return idx.astype(np.int64), dist


def test_goldens_are_there_and_tie():
    assert len(NAMES) >= 20, NAMES
    g = kc.load("ref_kdtree_dense_120x160.npz")
    d = g["depth_xy"]
    # a brute-force lowest-index search disagrees with the reference on many tied queries: the goldens discriminate
    q = g["queries"]
    lowest = np.concatenate([np.argmin(((q[s:s + 512, None, :] - d[None]) ** 2).sum(-1), axis=1) for s in range(0, len(q), 512)])
    assert (lowest != g["ref_idx"]).sum() > 500
    assert np.array_equal(g["ref_dist"], np.sqrt(((q - d[g["ref_idx"]]) ** 2).sum(1)))


def test_known_answer_4x4():
    """4 x 4 points at even coordinates, inserted row by row: the reference returns point 5 = (2, 2) for (1, 1), (3, 1) and (1, 3) —
    four points tie at sqrt(2) each time, and a lowest-index rule would return 0, 1 and 4."""
    import pyoracle as po
    g = kc.load("ref_kdtree_grid4x4_row_major.npz")
    assert g["queries"][:3].tolist() == [[1, 1], [3, 1], [1, 3]]
    assert g["ref_idx"][:3].tolist() == [5, 5, 5]
    assert po.kdtree_nn(g["depth_xy"], g["queries"][:3])[0].tolist() == [5, 5, 5]


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_reference_tree(po, name):
    g = kc.load(name)
    idx, dist = po.kdtree_nn(g["depth_xy"], g["queries"])
    assert np.array_equal(idx, g["ref_idx"]), f"{(idx != g['ref_idx']).sum()} of {len(idx)} queries differ"
    assert np.array_equal(dist, g["ref_dist"])


@pytest.mark.parametrize("name", NAMES)
def test_product_tree_equals_reference_tree(hl, name):
    g = kc.load(name)
    idx, dist = host_walk(hl, g["depth_xy"], g["queries"])
    assert np.array_equal(idx, g["ref_idx"]), f"{(idx != g['ref_idx']).sum()} of {len(idx)} queries differ"
    assert np.array_equal(dist, g["ref_dist"])


@pytest.mark.parametrize("kind", ["fma", "swap"])
def test_near_tie_goldens_need_separate_rounding(kind):
    """The near-tie goldens would fail a search that contracts `dist += dy*dy` into an FMA: at every site the reference's winner is
    not the point such a search prefers."""
    g = kc.load(f"ref_kdtree_near_tie_{kind}.npz")
    xy, q = g["depth_xy"], g["queries"]
    flips = sum(kc.contracted_winner(xy, q[k], [2 * k, 2 * k + 1]) != g["ref_idx"][k] for k in range(len(q)))
    assert flips == len(q) if kind == "fma" else flips > len(q) // 4


def test_oracle_set_depth_map_uses_the_tree(po):
    import np_keyframe_oracle as ko
    g = kc.load("ref_kdtree_every_other_120x160.npz")
    di = np.arange(1, len(g["depth_xy"]) + 1, dtype=np.float64)
    idp, _ = ko.set_depth_map(g["queries"], g["depth_xy"], di, 1.0, 3.0)
    assert np.array_equal(idp, di[g["ref_idx"]])


def _fuzz_case(rng, t):
    kind = t % 6
    if kind == 0:                                   # dense grid with holes
        H, W = rng.integers(2, 48, 2)
        xy = kc.grid_points(kc.holes_mask(rng, H, W, rng.uniform(0, 0.6)))
    elif kind == 1:                                 # every other pixel / every third
        H, W = rng.integers(3, 60, 2)
        xy = kc.grid_points(kc.holes_mask(rng, H, W, rng.uniform(0, 0.4), step=int(rng.integers(2, 4))))
    elif kind == 2:                                 # duplicates
        H, W = rng.integers(2, 30, 2)
        b = kc.grid_points(kc.holes_mask(rng, H, W, 0.3))
        xy = np.concatenate([b, b[rng.integers(0, max(1, len(b)), len(b))]]) if len(b) else b
        xy = xy[rng.permutation(len(xy))]
    elif kind == 3:                                 # tiny m
        H, W = 8, 8
        xy = rng.integers(0, 6, (int(rng.integers(1, 6)), 2)).astype(np.float64)
    elif kind == 4:                                 # real-valued near-ties
        H, W = 20, 26
        xy, _ = kc.near_tie_lattice(rng, H, W, 5, ["sqrt", "swap"][t % 2])
    else:                                           # integer cloud, heavy ties
        H, W = rng.integers(4, 40, 2)
        xy = rng.integers(0, [W, H], (int(rng.integers(1, 400)), 2)).astype(np.float64)
    if len(xy) == 0:
        xy = np.array([[0.0, 0.0]])
    return xy, kc.frame_queries(H + 2, W + 2) - 1.0


def test_fuzz_oracle_and_product_equal_reference_tree(po, hl):
    if not refcase.kdtree_available():
        pytest.skip("oracle/_ref/kdtree_nn is not built here (no reference tree): the golden cases above still pin f4")
    rng = np.random.default_rng(7)
    for t in range(300):
        xy, q = _fuzz_case(rng, t)
        ri, rd = refcase.kdtree_nn(xy, q)
        oi, od = po.kdtree_nn(xy, q)
        hi, hd = host_walk(hl, xy, q)
        assert np.array_equal(oi, ri) and np.array_equal(od, rd), f"oracle, case {t} (m = {len(xy)})"
        assert np.array_equal(hi, ri) and np.array_equal(hd, rd), f"product walk, case {t} (m = {len(xy)})"
