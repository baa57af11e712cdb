"""csrc/eds_immdepth.hpp (namespace edsimd: the loop of include/eds_hip_immdepth.h, what the device kernels run) compiled with g++ and
compared bit for bit with (1) an independent numpy statement of the loop — brute-force nearest where the nearest point is unique, the
pinned tree walk where it is not — and (2) edskd::nn and edsimm::construct composed by hand.  No GPU needed."""
import numpy as np
import pytest

import immdepth_cases as dc
import immdepth_harness as dh
import np_immature_oracle as no
import np_immdepth_oracle as do

NAMES = sorted(dc.cases())
FIELDS = ("color", "weights", "gradH", "energyTH", "u", "v", "type")
STATE = ("idepth_min", "idepth_max", "quality", "last_uv", "last_interval", "status")


@pytest.fixture(scope="module")
def hl():
    return dh.load_harness()


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    if a.dtype.kind == "f":
        return (a.view(f"u{a.dtype.itemsize}") == b.view(f"u{a.dtype.itemsize}")) | (np.isnan(a) & np.isnan(b))
    return a == b


def _run(hl, c):
    tree = dh.tree_of(hl, c.xy, c.idp)
    pts, nn = dh.seed(hl, c.image, no.params(), tree, c.uv, c.type, c.scale)
    return tree, pts, nn


@pytest.mark.parametrize("name", NAMES)
def test_loop_equals_the_numpy_statement(hl, name):
    c = dc.cases()[name]
    tree, pts, nn = _run(hl, c)
    ref, rnn, unique = do.seed(c.image, c.xy, c.idp, c.uv, c.type, c.scale, perm=tree[0])
    assert unique.all() != c.ties, "the case's ties flag says whether brute force alone decides"
    for f in ("index", "idepth", "distance"):
        assert _bits(nn[f], rnn[f]).all(), (name, f)
    live = ref["alive"]
    assert np.array_equal(pts["alive"] != 0, live)
    for f in FIELDS:
        assert no.same_bits(pts[f][live], ref[f][live]).all(), (name, f)
    for f in STATE:
        assert no.same_bits(pts[f], ref[f]).all(), (name, f)


@pytest.mark.parametrize("name", NAMES)
def test_loop_equals_nn_and_construct_composed_by_hand(hl, name):
    c = dc.cases()[name]
    tree, pts, nn = _run(hl, c)
    pts2, nn2 = dh.composed(hl, c.image, no.params(), tree, c.uv, c.type, c.scale)
    assert pts.tobytes() == pts2.tobytes()
    for f in nn:
        assert _bits(nn[f], nn2[f]).all(), (name, f)


def test_the_cases_hold_what_they_are_named_for(hl):
    cs = dc.cases()
    st = lambda name: _run(hl, cs[name])[1]
    p = st("distance_one")
    assert p["alive"].all()
    assert p["status"].tolist() == [no.GOOD, no.UNINITIALIZED, no.GOOD, no.UNINITIALIZED, no.GOOD, no.UNINITIALIZED]
    d = _run(hl, cs["distance_one"])[2]["distance"]
    assert d[0] == d[2] == d[4] == 1.0 and (d[1::2] > 1.0).all() and (d[1::2] < 1.0 + 1e-14).all()
    # the interval of a GOOD point: idepth -+ 0.1 * distance formed in fp64, narrowed
    assert p["idepth_min"][0] == np.float32(np.float64(np.float32(0.5)) - 0.1 * 1.0) and p["idepth_max"][0] == np.float32(np.float64(np.float32(0.5)) + 0.1 * 1.0)
    # pixels whose pattern leaves the image are dead in every random list, and both statuses occur among the living
    for name in (n for n in NAMES if n != "distance_one"):
        p = st(name)
        assert (p["alive"] == 0).any(), name
    p = st("random_1000")
    live = p["alive"] != 0
    assert (p["status"][live] == no.GOOD).any() and (p["status"][live] == no.UNINITIALIZED).any()
    # the grid map and the 4 097-point map are the host's to build; random real-valued maps up to 4 096 points are the device's
    assert not dh.device_builds(hl, cs["grid"].xy) and not dh.device_builds(hl, cs["random_4097"].xy)
    assert all(dh.device_builds(hl, cs[f"random_{m}"].xy) for m in dc.SIZES if m <= 4096)
    # ties: a pixel between its two points, at 0.5 from each
    nn = _run(hl, cs["ties"])[2]
    assert (nn["distance"][::3] <= 0.5).all() and (nn["distance"][::3] == 0.5).sum() >= 30
    # scale: the distance is taken against the unscaled pixel, so it differs from the walk's own minimum distance
    c = cs["scaled"]
    tree = dh.tree_of(hl, c.xy, c.idp)
    a = dh.nearest(hl, tree, c.uv, c.scale)
    q = do.query(c.uv, c.scale)
    own = np.sqrt(((q - tree[1][a["pos"]]) ** 2).sum(axis=1))
    assert (np.abs(a["distance"] - own) > 1.0).any()
    # a negative and a NaN inverse depth reach a living GOOD point unchanged
    c = cs["odd_idepth"]
    pts, nn = _run(hl, c)[1:]
    good = (pts["alive"] != 0) & (pts["status"] == no.GOOD)
    assert (good & (nn["idepth"] < 0)).any() and (good & np.isnan(nn["idepth"])).any()
    assert np.isnan(pts["idepth_min"][good & np.isnan(nn["idepth"])]).all()
    # an empty map is the first constructor
    c = cs["empty"]
    pts, nn = _run(hl, c)[1:]
    assert (pts["status"] == no.UNINITIALIZED).all() and (nn["index"] == -1).all() and np.isnan(pts["idepth_max"]).all()


def test_standalone_program_runs_the_cases_and_degenerate_inputs():
    """the program a sanitizer build runs (python tests/immdepth_harness.py -fsanitize=address,undefined), here built plainly"""
    out = dh.run_standalone(list(dc.cases().values()), lambda c: no.params())
    assert f"{len(NAMES)} cases" in out and " 0 mismatches" in out, out
