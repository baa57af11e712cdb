"""csrc/eds_activate.hpp (namespace edsact, compiled with plain g++) against tests/np_activate_oracle.py, bit for bit with any NaN equal
to any NaN, on every output: the map after seeding, the map after the selection, the fates, the fitted inverse depths, the sums, the
residuals' states and energies and the points that leave.  The oracle runs the literal list form of growDistBFS, edsact the round form.
The cases must discriminate on the oracle alone: every branch the header names occurs, every mutation changes a case, and no
comparison of the committed cases is within 4 ulps of its threshold.  No GPU needed."""
import numpy as np
import pytest

import activate_cases as ac
import activate_harness as ah
import np_activate_oracle as ao
import np_immature_oracle as no

CASES = list(ac.cases())
HUBER = float(no.params()["huber_th"])


@pytest.fixture(scope="module")
def hl():
    return ah.load_harness()


def assert_same(a, b, what):
    same = no.same_bits(np.asarray(a), np.asarray(b))
    assert same.all(), f"{what}: {int((~same).sum())} of {same.size} differ, first at {np.argwhere(~same)[0]}"


def compare(got, want, name):
    assert_same(got["map_seeded"], want["map_seeded"], f"{name} map after seeding")
    assert_same(got["map_selected"], want["map_selected"], f"{name} map after selection")
    for h in range(len(want["fates"])):
        assert_same(got["fates_selected"][h], want["fates_selected"][h], f"{name} host {h} fates after selection")
        assert_same(got["fates"][h], want["fates"][h], f"{name} host {h} fates")
        for k in ("idepth", "energy", "hdd", "bd", "res_state", "res_energy"):
            assert_same(got["results"][h][k], want["results"][h][k], f"{name} host {h} {k}")


@pytest.mark.parametrize("name", CASES)
def test_edsact_equals_the_oracle(hl, name):
    c = ac.cases()[name]
    want = ac.oracle_run(name)
    got = ah.run_case(hl, c, want["prm"], HUBER)
    compare(got, want, name)
    for h in range(c.F):
        assert_same(got["alive"][h], want["points"][h]["alive"], f"{name} host {h} alive")
    assert got["counts"].sum() == sum(int(p["alive"].sum()) for i, p in enumerate(c.P) if i != c.newest)


def test_the_cases_take_every_branch():
    fates = np.concatenate([f for n in CASES for f in ac.oracle_run(n)["fates"]])
    sel = np.concatenate([f for n in CASES for f in ac.oracle_run(n)["fates_selected"]])
    for f in (ao.DELETED_UNTRACED, ao.DELETED_CANNOT, ao.KEPT_CANNOT, ao.DELETED_OUT_OF_MAP, ao.KEPT_TOO_CLOSE, ao.KEPT_WEAK, ao.DROPPED, ao.ACTIVATED):
        assert (fates == f).any(), ao.FATE_NAMES[f]
    assert (sel == ao.CHOSEN).any() and not (fates == ao.CHOSEN).any()
    st = {k: sum(ac.oracle_run(n)["stats"][k] for n in CASES) for k in ac.oracle_run(CASES[0])["stats"]}
    for k in ("accept", "reject", "step_break", "weak_first", "weak_loop", "dropped_few_in", "oob_late_tap", "outlier_slack1_only"):
        assert st[k] > 0, (k, st)
    assert st["undecided"] == 0, st


def test_the_maps_have_the_stated_shapes():
    w = ac.oracle_run("w64_f3")["map_seeded"]
    h1, w1 = w.shape
    inner = w.copy()
    inner[[0, 0, -1, -1], [0, -1, 0, -1]] = 0          # a corner is reached only from its diagonal neighbour, and only in an odd round
    assert (w1, h1) == (32, 24) and (inner < 1000).all()
    assert (w[:, 1] == 0).any() and (w[:, w1 - 1] == 0).any() and (w[h1 - 1, :] == 0).any()
    assert not (w[:, 0] == 0).any() and not (w[0, :] == 0).any()
    far = ac.oracle_run("corner_f3_gn0")["map_seeded"]
    assert far.shape == (96, 128) and (far == 1000).any() and (far == 39).any()
    assert (ac.oracle_run("w64_f2_noactive")["map_seeded"] == 1000).all()
    vals = np.unique(np.concatenate([ac.oracle_run(n)["map_selected"].ravel() for n in CASES]))
    assert set(vals.tolist()) <= set(range(40)) | {1000}


def _differs(a, b):
    keys = ("map_seeded", "map_selected")
    if any(not no.same_bits(a[k], b[k]).all() for k in keys):
        return True
    for h in range(len(a["fates"])):
        if not (a["fates"][h] == b["fates"][h]).all():
            return True
        if any(not no.same_bits(a["results"][h][k], b["results"][h][k]).all() for k in ("idepth", "energy", "hdd", "bd", "res_state", "res_energy")):
            return True
    return False


@pytest.mark.parametrize("mutation, where", [
    (dict(even8=True), "w64_f3"), (dict(expand_ring=True), "w64_f3"), (dict(rounds=41), "corner_f3_gn0"), (dict(reverse_hosts=True), "corner_f3_gn0"),
    (dict(div_floor=True), "w64_f3_frac"), (dict(discard_partial=True), "m96_f8_obs3"), (dict(pre0=True), "w64_f3"),
])
def test_every_mutation_changes_a_case(mutation, where):
    assert _differs(ac.oracle_run(where), ac.oracle_run(where, **mutation)), mutation


def test_the_finite_test_on_the_old_energy_is_not_separable():
    """the loop tests isfinite on the OLD E; an input that separates it from a test on E' needs an E that is finite with an E' that is
    not (or the reverse) — the energies are sums of clamped, finite terms, so no reachable input does"""
    assert sum(ac.oracle_run(n)["stats"]["finite_test_differs"] for n in CASES) == 0


def test_the_round_form_equals_the_list_form_from_one_seed(hl):
    """addIntoDistFinal on a map that already holds values: never above what it was, never below the minimum over unobstructed
    grows from every seed (it is NOT that minimum in general: a path can be cut)"""
    c = ac.cases()["corner_f3_gn0"]
    want = ac.oracle_run("corner_f3_gn0")
    w1, h1 = c.W >> 1, c.H >> 1
    chosen = [(h, i) for h in range(c.F) for i in np.flatnonzero(want["fates_selected"][h] == ao.CHOSEN)]
    assert len(chosen) >= 2
    seeded, selected = want["map_seeded"], want["map_selected"]
    cells = []
    for h, i in chosen:
        P = c.P[h]
        cell, _ = ao._cell(c.KRKi1[h], c.Kt1[h], P["u"][i], P["v"][i], np.float32(0.5) * (P["idepth_max"][i] + P["idepth_min"][i]), w1, h1)
        cells.append(cell)
    naive = seeded.copy()
    for x, y in cells:                     # the Chebyshev / city-block mix of an unobstructed grow, cut at 39
        m = [1000] * (w1 * h1)
        m[x + w1 * y] = 0
        ao.grow(m, w1, h1, [(x, y)])
        naive = np.minimum(naive, ao.map_array(m, w1, h1))
    assert (selected <= seeded).all() and (selected >= naive).all()


def test_params_defaults_and_validity(hl):
    raw = np.zeros(6, np.float32)
    hl.act_params_default(raw.ctypes.data_as(ah._vp))
    assert raw.tobytes() == ah.pack_params(ao.params())
    assert hl.act_params_valid(ah.pack_params(ao.params())) == 1
    for bad in (dict(gn_its_on_point_activation=17), dict(gn_its_on_point_activation=-1), dict(min_obs=-1), dict(scale_idepth=0.0),
                dict(min_idepth_h_act=np.nan), dict(max_trace_pixel_interval=np.inf)):
        assert hl.act_params_valid(ah.pack_params(ao.params(**bad))) == 0, bad
