"""The scene of tests/cycle_cases.py holds what it is for: the host route of tests/cycle_harness.py (the g++ restatements alone, no GPU)
run over the four keyframe cycles meets every condition below, so that tests/test_cycle_gpu.py compares the device with a chain in
which points live a whole life, slots are refilled, history columns are lowered and cleared and Gauss-Newton steps are accepted and
rejected.

Measured on the host chain (points / residuals in the window at step 13; marginalised, dropped, kept at step 5; activated; residuals
towards the new keyframe): the figures are in DESIGN.md §23a and asserted here as lower bounds only; the peaks are asserted exactly,
because tests/test_cycle_gpu.py opens its handles with them."""
import numpy as np
import pytest

import cycle_cases as cc
import cycle_harness as ch


@pytest.fixture(scope="module")
def run():
    snaps, peaks = ch.run("host")
    return snaps, peaks


def _step(snaps, cycle, step):
    return next(s for s in snaps if s["cycle"] == cycle and s["step"] == step)


def _keys(snap):
    """a point's identity across gathers and slot shifts: (the global index of its host frame, u, v)"""
    rows = snap["tables"]["rows"]
    return [(snap["frames"][h], float(u), float(v)) for h, (u, v) in zip(rows["host"], rows["uv"])]


def test_every_cycle_marginalises_drops_keeps_activates_and_inserts(run):
    snaps, _ = run
    assert len(snaps) == cc.CYCLES * ch.STEPS
    for k in range(1, cc.CYCLES + 1):
        kept, marginalised, dropped = _step(snaps, k, 5)["out"]["fate_counts"][:3]
        assert marginalised >= 1 and dropped >= 1 and kept >= 10, (k, kept, marginalised, dropped)
        assert _step(snaps, k, 6)["out"]["res_m"] >= 1
        assert _step(snaps, k, 7)["out"]["left"][0] == marginalised + dropped
        assert _step(snaps, k, 12)["out"]["inserted"][0] >= 3 and _step(snaps, k, 12)["out"]["inserted"][1] >= 3
        assert _step(snaps, k, 13)["out"]["inserted"] >= 1
        assert _step(snaps, k, 10)["out"]["map_n"] >= 10 and _step(snaps, k, 10)["out"]["alive"].sum() >= 30


def test_activated_points_live_a_whole_life(run):
    """points that entered through insert_activated in cycle k leave by the flags of a later cycle, one of them hosted by a keyframe
    that came in through the second or a later refill of slot F - 1"""
    snaps, _ = run
    born = {}
    for k in range(1, cc.CYCLES + 1):
        for key in set(_keys(_step(snaps, k, 12))) - set(_keys(_step(snaps, k, 11))):
            born[key] = k
    left = []
    for k in range(2, cc.CYCLES + 1):
        gone = set(_keys(_step(snaps, k, 6))) - set(_keys(_step(snaps, k, 7)))
        left += [(key, born[key], k) for key in gone if key in born and born[key] < k]
    assert len(left) >= 5, len(left)
    assert any(key[0] >= cc.F + 1 for key, _, _ in left), sorted({key[0] for key, _, _ in left})


def test_steps_are_accepted_and_rejected(run):
    snaps, _ = run
    accepted = np.concatenate([_step(snaps, k, 2)["out"]["accepted"] for k in range(1, cc.CYCLES + 1)])
    assert (accepted == 1).any() and (accepted == 0).any(), accepted
    for k in range(1, cc.CYCLES + 1):
        for sol in _step(snaps, k, 2)["out"]["solves"]:
            assert np.isfinite(sol["x"]).all() and sol["res_in_a"] > 0


def test_every_residual_state_occurs_after_an_edit(run):
    """the tables of cycles 2 .. 4 have been through every edit of the cycle before"""
    snaps, _ = run
    seen = np.zeros(3, np.int64)
    for k in range(2, cc.CYCLES + 1):
        seen += np.bincount(_step(snaps, k, 3)["tables"]["residuals"]["state"], minlength=3)
    assert (seen > 0).all(), seen
    lin = sum(int(_step(snaps, k, 13)["tables"]["state"]["is_linearized"].sum()) for k in range(1, cc.CYCLES))
    assert lin > 0                                                                                    # linearized residuals survive a whole cycle's gathers


def test_last_target_holds_cleared_lowered_and_unchanged_targets_at_once(run):
    snaps, _ = run
    found = []
    for k in range(1, cc.CYCLES + 1):
        before, after = _step(snaps, k, 7)["history"]["last_target"], _step(snaps, k, 8)["history"]["last_target"]
        assert before.shape == after.shape                                                            # a frame's marginalisation removes no point
        leaving = cc.LEAVING[k - 1]
        cleared, lowered, unchanged = (before == leaving) & (after == -1), (before > leaving) & (after == before - 1), (before >= 0) & (before < leaving) & (after == before)
        assert (cleared | lowered | unchanged | (before == -1)).all()
        found.append(bool(cleared.any() and lowered.any() and unchanged.any()))
    assert any(found), found


def test_the_buffer_parity_at_step_one_differs_between_cycles(run):
    """of the per-point pair of buffer sets and of the per-residual pair, each counted by the edits that exchange it on the device
    (cycle_harness.Driver.exchanged); without the remove_points that flags nothing in cycles 2 and 4 the per-point pair, exchanged
    twice a cycle, would start every cycle on the same side"""
    snaps, _ = run
    parity = np.array([_step(snaps, k, 1)["out"]["parity"] for k in range(1, cc.CYCLES + 1)])
    assert len(set(parity[:, 0])) == 2 and len(set(parity[:, 1])) == 2, parity
    for k in range(1, cc.CYCLES + 1):                                                                 # the no-op moved nothing
        assert tuple(_step(snaps, k, 4)["tables"]["counts"]) == (_step(snaps, k, 3)["tables"]["counts"][0], _step(snaps, k, 3)["tables"]["counts"][1] - _step(snaps, k, 4)["out"]["gone"])


def test_the_host_chain_repeats(run):
    snaps, peaks = run
    again, peaks2 = ch.run("host")
    assert ch.first_difference(snaps, again) is None and peaks == peaks2


def test_the_kept_points_are_no_worse_than_the_initial_ones(run):
    """a condition on the inputs, not a tolerance on the device: the scene is exact, so the optimisation must not drive the inverse
    depths away from the plane's"""
    snaps, _ = run
    c = cc.case()
    end = _step(snaps, cc.CYCLES, 13)
    rows = end["tables"]["rows"]
    err = c.idepth_error(end["frames"], rows["host"], rows["uv"], end["tables"]["state"]["idepth_scaled"])
    assert np.median(err) <= c.initial_error, (float(np.median(err)), c.initial_error)


def test_the_recorded_peaks_are_the_measured_ones(run):
    _, peaks = run
    assert (peaks["points"], peaks["residuals"], peaks["immature"]) == (cc.PEAK_POINTS, cc.PEAK_RESIDUALS, cc.PEAK_IMMATURE), peaks
