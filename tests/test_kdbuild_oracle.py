"""The sort-based k-d build against std::nth_element's (CPU only): the numpy restatement (tests/np_kdbuild_oracle.py), the product
header's serial restatement (slam-eds_amd/csrc/eds_kdbuild.hpp: the steps k_kd_build takes) and edskd::build_tree give the same index
array wherever the ambiguity rule says "unambiguous"; the rule flags every case it has to; and the cases the GPU tests call
device-built are unambiguous and within the capacity, so that no GPU test can pass through the host fallback.  Everything is exact."""
import ctypes as C

import numpy as np
import pytest

import kdbuild_cases as kc
import np_kdbuild_oracle as kd

from kdbuild_harness import header_sorted, host_tree, load_harness, walk


@pytest.fixture(scope="module")
def hl():
    return load_harness()


UNAMBIGUOUS = kc.unambiguous_cases()
AMBIGUOUS = kc.ambiguous_cases()


def test_capacity_and_bounds_arithmetic(hl):
    assert hl.kdb_capacity() == kc.CAPACITY >= 4096
    lo, hi = C.c_int(), C.c_int()
    for m in (1, 2, 3, 6, 7, 8, 100, 4096):
        D = hl.kdb_levels(m)
        assert D == int(m).bit_length()
        # every position becomes a node exactly once, at the level where it is the middle of its sub-range; after D levels none is left
        born = np.full(m, -1)
        for level in range(D + 1):
            for p in range(m):
                if hl.kdb_segment_of(m, level, p, C.byref(lo), C.byref(hi)):
                    assert lo.value <= p < hi.value and level < D
                    if p == lo.value + (hi.value - lo.value - 1) // 2:
                        assert born[p] == -1
                        born[p] = level
                else:
                    assert 0 <= born[p] < level
        assert (born >= 0).all()


@pytest.mark.parametrize("name,xy", UNAMBIGUOUS, ids=[n for n, _ in UNAMBIGUOUS])
def test_three_builds_agree_where_unambiguous(hl, name, xy):
    ref = host_tree(hl, xy)
    a, amb_a = kd.build_sorted(xy)
    b, amb_b = header_sorted(hl, xy)
    assert not amb_a and not amb_b, name
    assert np.array_equal(a, ref) and np.array_equal(b, ref), name
    assert sorted(ref.tolist()) == list(range(len(xy)))


def test_planted_maps_do_hold_duplicates():
    for s in range(3):
        xy = kc.planted_away(s)
        assert len(np.unique(xy[:, 0])) < len(xy) and len(np.unique(xy[:, 1])) < len(xy)


def test_projected_maps_are_what_the_gpu_projects():
    maps = kc.projected_maps()
    assert len(maps) == 4 and all(len(xy) >= 100 for _, xy in maps)


@pytest.mark.parametrize("name,xy", AMBIGUOUS, ids=[n for n, _ in AMBIGUOUS])
def test_rule_flags(hl, name, xy):
    assert kd.ambiguous(xy), name
    assert header_sorted(hl, xy)[1], name


def test_rule_is_not_trigger_happy(hl):
    """a duplicate far from every median, and the ambiguous cases with their duplicate removed, are not flagged"""
    base = kc.real_map(77, 101)
    assert not kd.ambiguous(base) and not header_sorted(hl, base)[1]
    z = dict(kc.ambiguous_cases())["signed-zero-median"].copy()
    z[3, 0] = 0.5
    assert not kd.ambiguous(z) and not header_sorted(hl, z)[1]


def test_flag_matters_on_integer_grids(hl):
    """among the ambiguous grids at least one array differs from nth_element's when the build goes on regardless"""
    differ = 0
    for name, xy in AMBIGUOUS:
        if not name.startswith("grid-holes"):
            continue
        forced, amb = kd.build_sorted(xy, force=True)
        assert amb and sorted(forced.tolist()) == list(range(len(xy)))
        differ += int(not np.array_equal(forced, host_tree(hl, xy)))
    assert differ >= 1


@pytest.mark.parametrize("name", ["real-2", "real-65", "real-1000", "dyadic-300", "planted-away-0", "projected-tall-own"])
def test_walk_over_the_sorted_tree_equals_the_oracle(hl, po, name):
    xy = dict(UNAMBIGUOUS)[name]
    perm, amb = header_sorted(hl, xy)
    assert not amb
    q = kc.tie_queries(xy, len(xy))
    pos, dist = walk(hl, kd.tree_order(xy, perm), q)
    ref_idx, ref_dist = po.kdtree_nn(xy, q)
    assert np.array_equal(perm[pos], ref_idx) and np.array_equal(dist, ref_dist)
    if name == "dyadic-300":                            # the midpoints do tie: two map points at exactly the winning distance
        d = np.sqrt(((q[:40, None, :] - xy[None]) ** 2).sum(-1))
        assert ((d == d.min(axis=1, keepdims=True)).sum(axis=1) >= 2).sum() >= 20


def test_device_built_cases_never_fall_back():
    """the condition that keeps a GPU test from passing through the host fallback: share of device-built cases that fall back = 0"""
    maps = kc.device_built_maps()
    fall_back = [n for n, xy in maps if kd.ambiguous(xy) or len(xy) > kc.CAPACITY]
    assert len(maps) >= 50 and fall_back == []
    for H, W in kc.FRAMES:                              # ... and the integer-grid keyframe map is what takes the host build
        assert kd.ambiguous(kc.keyframe_grid_map(1, H, W)[0])
