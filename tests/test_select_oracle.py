"""csrc/eds_pixsel.hpp (edspix, the text the device kernels run, here under g++ in its scan form) against the literal numpy oracle of
the reference's nested loop (tests/np_select_oracle.py), bit for bit, on the committed cases (tests/select_cases.py); that the cases
take every branch the header names, that each deliberate mistake in the oracle changes a case, that no comparison is decided within
4 ulps, and the sanitizer run of the stand-alone program.  No GPU: nothing here launches anything."""
import subprocess

import numpy as np
import pytest

import np_select_oracle as so
import select_cases as sc
import select_harness as sh

CASES = sc.cases()
_oracle = {}


def oracle_run(name):
    """the literal oracle over one case, computed once and shared: (result, stats, levels, ths, ths_s)"""
    if name not in _oracle:
        c = CASES[name]
        o = so.Selector(c.H, c.W, c.table, **c.prm)
        o.potential = c.potential
        o.set_image(c.image, c.B)
        r = o.make_maps(c.density, c.recursions, c.th_factor)
        _oracle[name] = (r, dict(o.stats), o.L, o.ths, o.ths_s)
    return _oracle[name]


def run_selector(s, c):
    s.potential = c.potential
    s.set_image(c.image, c.B)
    n = s.make_maps(c.density, c.recursions, c.th_factor, keep_pass_maps=True)
    uv, typ = s.selection()
    return dict(num_have_sub=n, map=s.map(), passes=s.passes, pass_maps=s.pass_maps, potential=s.potential, uv=uv, type=typ,
                levels=[s.level(l) for l in range(3)], ths=s.thresholds(0), ths_s=s.thresholds(1))


def assert_equals_oracle(got, name):
    """every output the selector has, bit for bit"""
    r, _, L, ths, ths_s = oracle_run(name)
    for l in range(3):
        assert got["levels"][l].shape == L[l].shape
        assert np.array_equal(got["levels"][l].view(np.uint32), L[l].view(np.uint32)), f"{name}: level {l}"
    assert np.array_equal(got["ths"].view(np.uint32), ths.view(np.uint32)), f"{name}: ths"
    assert np.array_equal(got["ths_s"].view(np.uint32), ths_s.view(np.uint32)), f"{name}: thsSmoothed"
    assert got["passes"] == r["passes"], f"{name}: potentials and n2, n3, n4 per pass"
    assert len(got["pass_maps"]) == len(r["pass_maps"])
    for k, (a, b) in enumerate(zip(got["pass_maps"], r["pass_maps"])):
        assert np.array_equal(a, b), f"{name}: the map after pass {k}"
    assert np.array_equal(got["map"], r["map"]), f"{name}: the map"
    assert got["num_have_sub"] == r["num_have_sub"] and got["potential"] == r["potential"], name
    assert np.array_equal(got["uv"], r["uv"]) and np.array_equal(got["type"].view(np.uint32), r["type"].view(np.uint32)), f"{name}: the selection list"
    assert set(np.unique(got["map"])) <= {0, 1, 2, 4}


@pytest.mark.parametrize("name", list(CASES))
def test_edspix_equals_the_literal_oracle(name):
    c = CASES[name]
    h = sh.HostSelector(c.H, c.W, c.table, **c.prm)
    assert_equals_oracle(run_selector(h, c), name)
    # a second call on the same image keeps the histograms and is makeMaps from the potential the first one left
    assert h.hist_valid
    r, _, L, _, _ = oracle_run(name)
    o = so.Selector(c.H, c.W, c.table, **c.prm)
    o.L, o.frame = L, object()
    o.potential = r["potential"]
    r2 = o.make_maps(c.density, c.recursions, c.th_factor)
    n2 = h.make_maps(c.density, c.recursions, c.th_factor)
    assert n2 == r2["num_have_sub"] and np.array_equal(h.map(), r2["map"]) and h.passes == r2["passes"] and h.potential == r2["potential"]


def test_the_cases_take_every_branch():
    tot = {}
    for name in CASES:
        for k, v in oracle_run(name)[1].items():
            tot[k] = tot.get(k, 0) + v
    for k in ("map_1", "map_2", "map_4", "recurse_smaller", "recurse_larger", "subselect", "no_subselect", "sub_removed", "dirnorm_ties",
              "ths_aliased", "ths_clamped"):
        assert tot.get(k, 0) > 0, k
    n3 = sum(p[2] for name in CASES for p in oracle_run(name)[0]["passes"])
    n4 = sum(p[3] for name in CASES for p in oracle_run(name)[0]["passes"])
    assert n3 > 0 and n4 > 0
    shapes = {(c.H, c.W) for c in CASES.values()}
    assert {(64, 96), (96, 64), (100, 70)} <= shapes            # (H, W)
    assert {1, 2, 3, 5, 40} <= {c.potential for c in CASES.values()}
    assert {1.0, 2.0} <= {c.th_factor for c in CASES.values()}
    assert any(c.B is not None for c in CASES.values()) and any(c.B is None for c in CASES.values())
    assert {0, 1} <= {c.prm.get("select_direction_distribution", 1) for c in CASES.values()}
    assert sum(oracle_run("flat")[0]["passes"][-1][1:]) == 0
    assert np.array_equal(CASES["odd_70x100_p1_ref"].table, sh.reference_pattern(70 * 100))
    # 4 pot does not divide the image; a potential of 40 makes one block larger than the image
    assert any(c.W % (4 * c.potential) and c.H % (4 * c.potential) for c in CASES.values())
    c = CASES["odd_70x100_p40"]
    assert 4 * c.potential > max(c.H, c.W)


def test_no_comparison_is_decided_within_4_ulps():
    for name in CASES:
        st = oracle_run(name)[1]
        assert st.get("undecided_ag", 0) == 0 and st.get("undecided_dirnorm", 0) == 0 and st.get("undecided_quotia", 0) == 0, (name, st)


def test_ambiguous_cells_occur_and_change_n2():
    """cells whose selection depends on the direction drawn: every cell of the pure ramps, some of the half ramp; resolving them
    against the table gives another n2 than the prefix sum over the certain cells alone"""
    for name, everyone in (("h_ramp_all_sensitive", True), ("v_ramp_all_sensitive", True), ("half_ramp_some_sensitive", False)):
        c = CASES[name]
        h = sh.HostSelector(c.H, c.W, c.table, **c.prm)
        h.potential = c.potential
        h.set_image(c.image, c.B)
        h.make_maps(c.density, 0, c.th_factor)
        amb, n2_certain = h.scan_info()
        n2 = h.passes[-1][1]
        assert amb > 0 and n2 != n2_certain and n2 > 0, (name, amb, n2, n2_certain)
        assert (n2_certain == 0) == everyone, name
        assert n2 == oracle_run(name)[0]["passes"][0][1] or c.recursions > 0
    c = CASES["tex_64x96_sub"]
    h = sh.HostSelector(c.H, c.W, c.table, **c.prm)
    run_selector(h, c)
    assert h.scan_info()[0] == 0


@pytest.mark.parametrize("mut", so.MUTATIONS)
def test_each_mistake_in_the_oracle_changes_a_case(mut):
    changed = []
    for name, c in CASES.items():
        r = oracle_run(name)[0]
        o = so.Selector(c.H, c.W, c.table, **c.prm)
        o.potential = c.potential
        o.L, o.frame = oracle_run(name)[2], object()
        m = o.make_maps(c.density, c.recursions, c.th_factor, mut=mut)
        if m["passes"] != r["passes"] or not np.array_equal(m["map"], r["map"]):
            changed.append(name)
    assert changed, mut


def test_decisions_where_the_reference_is_undefined():
    hl = sh.load_harness()
    # a potential past the image is one cell; any potential up to 2^30 is accepted
    c = CASES["odd_70x100_p40"]
    a, b = sh.HostSelector(c.H, c.W, c.table), sh.HostSelector(c.H, c.W, c.table)
    for s, pot in ((a, 100), (b, 1 << 30)):
        s.potential = pot
        s.set_image(c.image)
        s.make_maps(c.density, 0, 1.0)
    assert np.array_equal(a.map(), b.map()) and a.passes[0][1:] == b.passes[0][1:]
    # nothing selected: quotia = +inf, the potential falls to 1 and stays
    f = CASES["flat"]
    s = sh.HostSelector(f.H, f.W, f.table)
    s.set_image(f.image)
    assert s.make_maps(50.0, 5, 1.0) == 0 and s.potential == 1 and [p[0] for p in s.passes] == [3, 1]
    assert hl.sel_params_size() == 16


def test_standalone_program_is_clean_under_the_sanitizers():
    """the committed cases and the hostile inputs of select_harness.cpp's main, once, as a program of its own"""
    flags = ["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-g"]
    try:
        out = sh.run_standalone(list(CASES.values()), lambda c: so.params(**c.prm), flags)
    except subprocess.CalledProcessError as e:
        raise AssertionError(e.output)
    assert f"select: {len(CASES)} committed cases" in out and "hostile inputs" in out, out
    assert "runtime error" not in out and "AddressSanitizer" not in out, out
