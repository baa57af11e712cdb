"""eds_wed_insert_activated of csrc/eds_winedit.hpp under g++ (tests/winedit_harness.py), no GPU needed: on windows over the frames of
tests/activate_cases.py, fed with the activated points of the activation oracle, every row after the insert equals
Activation.window_tables() merged per host by the numpy oracle (a stable sort by host; it knows nothing of candidates, grids or scans);
a following linearize equals the fresh-window path; what does not fit is refused and changes nothing; the mutations are caught.
(eds_win_apply's EDS_ERR_STATE before that linearize is the device's own mark: tests/test_winedit_gpu.py.)"""
import functools

import numpy as np
import pytest

import activate_cases as ac
import np_activate_oracle as ao
import np_winedit_oracle as oracle
import winedit_cases as wec
import winedit_harness as weh
import winsolve_harness as wsh


def _diff(a, b):
    fa, fb = dict(wsh.flatten(a)), dict(wsh.flatten(b))
    assert fa.keys() == fb.keys(), sorted(set(fa) ^ set(fb))
    return [k for k in fa if not wsh.same_bits(fa[k], fb[k])]


def activated_of(name):
    c, o = ac.cases()[name], ac.oracle_run(name)
    return ao.activated(c.P, o["fates"], o["results"])


def lin_after(w, s):
    c = s.win
    energy, counts = w.linearize(c.F, c.precalc, c.th)
    r = w.residuals()
    J = r["J"].copy()
    J[r["new_state"] == 1] = 0
    return dict(energy=np.float64(energy), counts=counts, new_state=r["new_state"], new_energy=r["new_energy"], ret=r["linearize_return"], J=J)


@functools.lru_cache(maxsize=None)
def _run(name):
    s = wec.insert_case(name)
    w, sv = wsh.open_case(s)
    ed = weh.HostEdit(w)
    wec.prepare_insert(w, sv, s)
    before = weh.snapshot(w, sv, ed)
    inserted = ed.insert_activated(activated_of(name), s.F)
    after = weh.snapshot(w, sv, ed)
    nxt = lin_after(w, s)
    sv.close()
    w.close()
    return dict(before=before, after=after, inserted=inserted, next=nxt)


@pytest.mark.parametrize("name", wec.INSERT_NAMES)
def test_the_inserted_rows_equal_window_tables_merged_per_host(name):
    s = wec.insert_case(name)
    out = _run(name)
    pts, res = wec.tables_of(activated_of(name), s.F)
    want = oracle.insert(out["before"], pts, res)
    bad = _diff(want, out["after"])
    assert not bad, bad[:12]
    assert out["inserted"] == (len(pts["host"]), len(res["point"]))
    if name != "w64_f2_noactive":
        assert out["inserted"][0] > 0 and out["inserted"][1] > 0
        assert out["before"]["state"]["is_linearized"].any() and out["before"]["residuals"]["J"].any()       # rows that had to move unchanged
    host = out["after"]["rows"]["host"]
    assert (np.diff(host) >= 0).all() and (np.diff(out["after"]["rows"]["point"]) >= 0).all()


@pytest.mark.parametrize("name", wec.INSERT_NAMES)
def test_a_following_linearize_equals_the_fresh_window_path(name):
    s = wec.insert_case(name)
    c = s.win
    out = _run(name)
    t = oracle.tables(out["after"])
    w = wsh.HostWindow(c.H, c.W, c.F)
    w.set_calib(*c.K)
    w.set_frames(0, c.images)
    w.set_points(*t["points"])
    w.set_residuals(*t["residuals"])
    assert not _diff(lin_after(w, s), out["next"])
    w.close()


def test_what_does_not_fit_is_refused_and_changes_nothing():
    name = "w64_f3"
    s = wec.insert_case(name)
    w, sv = wsh.open_case(s)
    ed = weh.HostEdit(w)
    wec.prepare_insert(w, sv, s)
    before = weh.snapshot(w, sv, ed)
    K, R = _run(name)["inserted"]
    for cap in ((w.n + K - 1, w.m + R), (w.n + K, w.m + R - 1)):
        with pytest.raises(wsh.HostError) as e:
            ed.insert_activated(activated_of(name), s.F, *cap)
        assert e.value.code == wsh.STATE and not _diff(before, weh.snapshot(w, sv, ed))
    with pytest.raises(wsh.HostError) as e:                      # a selection over more hosts than the call says
        ed.insert_activated(activated_of(name), 2)
    assert e.value.code == wsh.INVALID and not _diff(before, weh.snapshot(w, sv, ed))
    assert ed.insert_activated(activated_of(name), s.F, w.n + K, w.m + R) == (K, R)
    sv.close()
    w.close()


@pytest.mark.parametrize("mutate", oracle.INSERT_MUTATIONS)
def test_every_mutation_of_the_insert_oracle_is_caught(mutate):
    caught = []
    for name in wec.INSERT_NAMES:
        out = _run(name)
        pts, res = wec.tables_of(activated_of(name), wec.insert_case(name).F)
        if _diff(oracle.insert(out["before"], pts, res, mutate), out["after"]):
            caught.append(name)
    assert caught, mutate
