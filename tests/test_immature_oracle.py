"""The immature points on the CPU (no GPU needed).  First the numpy oracle (tests/np_immature_oracle.py) alone: the cases of
tests/immature_cases.py must DISCRIMINATE — every status and branch occurs, and the choices the header pins (first index of the
minimum, repeated addition, fy in the caller's KRKi) change some point's fate when they are made the other way.  Then csrc/eds_immature.hpp,
the code the device kernels run, compiled with g++ (tests/immature_harness.py): equal to the oracle bit for bit (any NaN equal to any
NaN) on every case, every trace and every output."""
import numpy as np
import pytest

import immature_cases as ic
import immature_harness as ih
import np_immature_oracle as no

NAMES = list(ic.cases())


def _total(name, key):
    return sum(s[key] for step in ic.oracle_run(name)["stats"] for s in step)


def _flipped(name, **variant):
    """points of the case whose final state differs between the reference's rule and the variant"""
    a, b = ic.oracle_run(name)["after"][-1], ic.oracle_run(name, **variant)["after"][-1]
    n = 0
    for pa, pb in zip(a, b):
        d = np.zeros(len(pa["u"]), bool)
        for f in ic.FIELDS:
            d |= (~no.same_bits(pa[f], pb[f])).reshape(len(d), -1).any(axis=1)
        n += int(d.sum())
    return n


def test_cases_cover_the_shapes_the_issue_names():
    cs = ic.cases()
    assert {(c.W, c.H) for c in cs.values()} >= {(96, 72), (72, 96), (160, 120)}
    assert all(c.K4[0] != c.K4[1] and c.K4[2] != (c.W - 1) / 2 and c.K4[3] != (c.H - 1) / 2 for c in cs.values())
    assert {len(c.hosts) for c in cs.values()} >= {1, 3, 7}
    assert {len(h["uv"]) for c in cs.values() for h in c.hosts} >= {1, 63, 64, 65, 300}
    assert {no.params(**c.prm)["trace_gn_iterations"] for c in cs.values()} == {0, 3}
    assert all(len(c.targets) == 4 for c in cs.values())
    assert any(np.isnan(t).any() for c in cs.values() for t in c.targets)
    steps = {s for n in NAMES for step in ic.oracle_run(n)["stats"] for st in step for s in st["max_steps"]}
    assert {64, 65, 99} <= steps and min(steps) <= 3


def test_every_status_occurs_and_a_second_outlier_turns_oob():
    seen = np.zeros(6, np.int64)
    for n in NAMES:
        o = ic.oracle_run(n)
        for pts in o["after"]:
            for p in pts:
                seen += no.summary(p)
    assert (seen > 0).all(), dict(zip(no.STATUS_NAMES, seen))
    assert sum(_total(n, "outlier_twice") for n in NAMES) > 0
    # ... and such a point really went OUTLIER, then OOB
    o = ic.oracle_run("x3_gn3")
    went = [(a["status"] == no.OUTLIER) & (b["status"] == no.OOB) & a["alive"] for k in range(1, 4) for a, b in zip(o["after"][k], o["after"][k + 1])]
    assert sum(int(w.sum()) for w in went) > 0
    # dead points exist, and both constructors' branches on distance
    assert any((~p["alive"]).any() for n in NAMES for p in ic.oracle_run(n)["after"][0])
    seeded = ic.oracle_run("y7_gn3_seeded")["after"][0]
    assert any((p["status"] == no.GOOD).any() and (p["status"] == no.UNINITIALIZED).any() for p in seeded)


def test_every_branch_of_the_trace_occurs():
    tot = {k: sum(_total(n, k) for n in NAMES) for k in ("finite_max", "nonfinite_max", "horizontal", "vertical", "gn_back", "gn_break", "n_1e5")}
    assert all(v > 0 for v in tot.values()), tot


def test_intervals_narrow_along_the_path():
    o = ic.oracle_run("x3_gn3")
    p1, p4 = o["after"][1][0], o["after"][4][0]
    both = (p1["status"] == no.GOOD) & (p4["status"] == no.GOOD)
    w1, w4 = (p1["idepth_max"] - p1["idepth_min"])[both], (p4["idepth_max"] - p4["idepth_min"])[both]
    assert both.sum() > 50 and np.median(w4) < 0.5 * np.median(w1)


def test_the_pinned_choices_change_some_points_fate():
    assert _flipped("x3_gn3", argmin_le=True) > 0          # first index of the minimum: strict <
    assert all(_flipped(n, mul_step=True) > 0 for n in ("x3_gn3", "long99"))     # ptx by repeated addition, not i * dx
    assert all(_flipped(n, wrong_fy=True) > 0 for n in NAMES)                     # fx for fy in the caller's KRKi


@pytest.fixture(scope="module")
def hl():
    return ih.load_harness()


def test_header_defaults_and_validation(hl):
    buf = (np.zeros(12, np.float32)).tobytes()
    import ctypes as C
    raw = C.create_string_buffer(buf, 48)
    hl.imm_params_default(raw)
    assert raw.raw == ih.pack_params(no.params())
    assert hl.imm_params_valid(raw) == 1
    for k, bad in (("trace_stepsize", 0.0), ("max_pix_search", float("nan")), ("trace_gn_iterations", 17), ("trace_gn_iterations", -1),
                   ("huber_th", -1.0), ("trace_gn_threshold", float("inf")), ("outlier_th_sum_component", 0.0), ("min_trace_test_radius", -1)):
        assert hl.imm_params_valid(ih.pack_params(no.params(**{k: bad}))) == 0, k


@pytest.mark.parametrize("name", NAMES)
def test_header_equals_oracle_bit_for_bit(hl, name):
    c, o = ic.cases()[name], ic.oracle_run(name)
    prm = o["prm"]
    for img, ref in zip([h["image"] for h in c.hosts] + c.targets, o["host_images"] + o["target_images"]):
        assert no.same_bits(ih.make_image(hl, img), ref).all()
    pts = [ih.construct(hl, h["image"], h["uv"], h["type"], h["idepth"], h["distance"], prm) for h in c.hosts]
    for p, ref in zip(pts, o["after"][0]):
        live = ref["alive"]
        assert np.array_equal(p["alive"] != 0, live)
        assert np.isnan(p["energyTH"][~live]).all()
        for f in ("color", "weights", "gradH", "energyTH", "u", "v", "type"):
            assert no.same_bits(p[f][live], ref[f][live]).all(), f
    for k, step in enumerate(c.steps):
        for i, (KRKi, Kt, aff, _) in enumerate(step):
            ih.trace(hl, pts[i], c.targets[k], prm, KRKi, Kt, aff)
            ref = o["after"][k + 1][i]
            for f in ic.FIELDS:
                bad = ~no.same_bits(pts[i][f], ref[f])
                assert not bad.any(), (name, k, i, f, np.argwhere(bad)[:5].tolist())


def test_standalone_program_runs_the_cases_and_degenerate_inputs():
    """the program a sanitizer build runs, here built plainly: all cases, then NaN / inf / zero KRKi and Kt, hostile seeds,
    points on and beyond the border"""
    out = ih.run_standalone(list(ic.cases().values()), lambda c: no.params(**c.prm))
    assert f"{len(NAMES)} cases" in out and "dead" in out
