"""csrc/eds_winedit.hpp under g++ (tests/winedit_harness.py) against the numpy oracle of tests/np_winedit_oracle.py, which gathers a
snapshot by the surviving indices and knows nothing of scans: on every window of tests/winsolve_cases.py, driven through linearize ->
apply -> set_state -> fix_linearization -> backup -> solve -> step, every row a caller can read equals the gathered snapshot bit for
bit after every step of every flag pattern of tests/winedit_cases.py, and the counts equal the oracle's; the edited window then
behaves as a fresh window built from the oracle's tables; the window's host copies follow the same rule; every mutation of the oracle
is caught (no GPU needed: nothing here launches anything)."""
import copy
import functools

import numpy as np
import pytest

import np_winedit_oracle as oracle
import winedit_cases as wec
import winedit_harness as weh
import winsolve_cases as wsc
import winsolve_harness as wsh

NAMES = list(wsc.ROUNDS)


def _diff(a, b):
    fa, fb = dict(wsh.flatten(a)), dict(wsh.flatten(b))
    assert fa.keys() == fb.keys(), sorted(set(fa) ^ set(fb))
    return [k for k in fa if not wsh.same_bits(fa[k], fb[k])]


def _open(s):
    w, sv = wsh.open_case(s)
    return w, sv, weh.HostEdit(w)


@functools.lru_cache(maxsize=None)
def _run(name, pattern, no_fix=False):
    """(snapshots, HM, bM, what the edited window does next) of the host restatement"""
    s = wec.cases()[name]
    if no_fix:
        s = copy.copy(s)
        s.fix = np.zeros_like(s.fix)
    w, sv, ed = _open(s)
    snaps, HM, bM = weh.run_pattern(w, sv, ed, s, pattern, wec.steps)
    after = weh.after_edit(w, sv, s, HM, bM, full=no_fix)
    sv.close()
    w.close()
    return snaps, HM, bM, after


def _expected(name, pattern, snaps, mutate=None):
    """the oracle's snapshot after every step, each from the snapshot the restatement gave before that step"""
    s = wec.cases()[name]
    rows = snaps[0]["rows"]
    out = []
    for k, (kind, flags) in enumerate(wec.steps(pattern, s, int(snaps[0]["counts"][0]), int(snaps[0]["counts"][1]), rows["host"], rows["point"])):
        before = snaps[k]
        e = oracle.edit(before, point_flag=flags, mutate=mutate) if kind == "points" else oracle.edit(before, select=flags, mutate=mutate)
        gone = before["counts"] - e["counts"]
        e["removed"] = gone if kind == "points" else gone[1:]
        out.append(e)
    return out


@pytest.mark.parametrize("pattern", wec.PATTERNS)
@pytest.mark.parametrize("name", NAMES)
def test_every_row_equals_the_snapshot_gathered_by_the_oracle(name, pattern):
    snaps, _, _, _ = _run(name, pattern)
    want = _expected(name, pattern, snaps)
    assert len(want) == len(snaps) - 1 >= 1
    for k, e in enumerate(want):
        got = {key: v for key, v in snaps[k + 1].items()}
        bad = _diff(e, got)
        assert not bad, (k, bad[:12])
    if pattern == "all":
        assert snaps[-1]["counts"].tolist() == [0, 0]
    if pattern == "none":
        assert not _diff({k: v for k, v in snaps[0].items()}, {k: v for k, v in snaps[-1].items() if k != "removed"})


def test_the_patterns_cover_what_they_claim():
    s = wec.cases()["f8_1100"]
    snaps, _, _, _ = _run("f8_1100", "null_select")
    st = snaps[0]["residuals"]["state"]
    assert (st == 1).any() and (st == 2).any() and (st == 0).any() and (snaps[1]["residuals"]["state"] == 0).all()
    assert snaps[1]["counts"][0] == snaps[0]["counts"][0]                       # points are never removed there
    snaps, _, _, _ = _run("f8_1100", "empty_run")
    first = snaps[1]["rows"]["res_first"]
    assert (np.diff(first) == 0).sum() >= 3 and (np.diff(snaps[2]["rows"]["res_first"]) == 0).any()
    for pat, host in (("host0", 0), ("host_last", 7)):
        snaps, _, _, _ = _run("f8_1100", pat)
        assert snaps[0]["per_host"][host] > 0 and snaps[1]["per_host"][host] == 0 and snaps[1]["counts"][0] > 0
    snaps, _, _, _ = _run("f8_1100", "random30")
    assert 0.2 < 1 - snaps[1]["counts"][0] / snaps[0]["counts"][0] < 0.4
    assert s.marg.any() and s.fix.any()
    lin = _run("f8_1100", "marginalised")[0]
    assert lin[1]["state"]["is_linearized"].any() and lin[1]["state"]["step"].any() and lin[1]["rows"]["idepth_backup"].any()
    assert lin[1]["residuals"]["J"].any() and lin[1]["state"]["res_toZeroF"].any()


@pytest.mark.parametrize("pattern", wec.PATTERNS)
@pytest.mark.parametrize("name", NAMES)
def test_the_edited_window_behaves_as_a_fresh_window_of_the_oracles_tables(name, pattern):
    """no residual is linearized here (a fresh window cannot be given such flags: that is what the edit is for), except, for
    "marginalised", the residuals of the marginalised points, which leave"""
    s = wec.cases()[name]
    snaps, HM, bM, after = _run(name, pattern, True)
    want = _expected(name, pattern, snaps)[-1]
    t = oracle.tables(want)
    c = s.win
    w = wsh.HostWindow(c.H, c.W, c.F)
    if c.prm:
        w.set_params(**c.prm)
    w.set_calib(*c.K)
    w.set_frames(0, c.images)
    w.set_points(*t["points"])
    w.set_residuals(*t["residuals"])
    sv = wsh.HostSolver(w)
    sv.set_state(s.F, c.adH, c.adT, s.delta, s.prior, s.delta_prior, s.cPrior, s.cDelta, want["state"]["priorF"], want["rows"]["deltaF"])
    fresh = weh.after_edit(w, sv, s, HM, bM, full=True)
    sv.close()
    w.close()
    bad = _diff(fresh, after)
    assert not bad, bad[:12]


@pytest.mark.parametrize("name", ["f3_5", "f8_1100"])
def test_the_host_copies_follow_the_same_flags(name):
    snaps, _, _, _ = _run(name, "random30")
    rows = snaps[0]["rows"]
    flag = wec.steps("random30", wec.cases()[name], int(snaps[0]["counts"][0]), int(snaps[0]["counts"][1]), rows["host"], rows["point"])[0][1]
    keep_p = (flag == 0).astype(np.int32)
    keep_r = keep_p[rows["point"]]
    host, point, target, max_host, max_target = weh.edit_mirrors(rows["host"], rows["point"], rows["target"], keep_p, keep_r)
    after = snaps[1]["rows"]
    assert wsh.same_bits(host, after["host"]) and wsh.same_bits(point, after["point"]) and wsh.same_bits(target, after["target"])
    assert max_host == after["host"].max() and max_target == after["target"].max()
    host, point, target, _, _ = weh.edit_mirrors(rows["host"], rows["point"], rows["target"], None, keep_r)
    assert wsh.same_bits(host, rows["host"]) and wsh.same_bits(point, rows["point"][keep_r != 0])


@pytest.mark.parametrize("mutate", oracle.MUTATIONS)
def test_every_mutation_of_the_oracle_is_caught(mutate):
    caught = []
    for name in NAMES:
        for pattern in wec.PATTERNS:
            snaps, _, _, _ = _run(name, pattern)
            try:
                want = _expected(name, pattern, snaps, mutate)
            except (IndexError, ValueError):                     # a mutation may leave an index outside its table
                caught.append((name, pattern))
                continue
            if any(_diff(e, snaps[k + 1]) for k, e in enumerate(want)):
                caught.append((name, pattern))
    assert caught, mutate
