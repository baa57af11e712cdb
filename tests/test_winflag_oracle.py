"""csrc/eds_winflag.hpp under g++ (tests/winflag_harness.py) against the literal numpy statement (tests/np_winflag_oracle.py) on the
windows of tests/winflag_cases.py: every column and every count bit for bit after the fixLinearization pass, after residuals and
points leave, after a frame leaves, after makeKeyFrame's insert and for activated points, and every fate and count of
flagPointsForRemoval's decisions; the case set reaches every branch (asserted, so a degenerate case set fails); an edited history behaves as one set afresh; every mutation of the oracle is caught (no GPU needed:
nothing here launches anything)."""
import numpy as np
import pytest

import np_winflag_oracle as oracle
import winflag_cases as wfc
import winflag_harness as wfh
import winsolve_harness as wsh

NAMES = wfc.NAMES


def _diff(a, b):
    fa, fb = dict(wsh.flatten(a)), dict(wsh.flatten(b))
    assert fa.keys() == fb.keys(), sorted(set(fa) ^ set(fb))
    return [k for k in fa if not wsh.same_bits(fa[k], fb[k])]


def _sequence(name, impl, mutate=None):
    """one keyframe's worth of calls on case `name` by `impl` (the oracle or the harness): everything each call returns"""
    c = wfc.case(name)
    kw = {} if mutate is None else dict(mutate=mutate)
    out = {}
    args = (c.host, c.uv, c.ids, c.point, c.target, c.state, c.active, c.precalc, c.F)
    out["keep_flags"] = impl.apply_fixed(c.history, *args, 0, **kw)[:2]
    h, counts = impl.apply_fixed(c.history, *args, 1, **kw)[:2]
    out["clear_flags"] = (h, counts)
    # DSO's toRemove loop: every residual that is not IN leaves
    keep = (c.state == 0).astype(np.int32)
    h = impl.remove_residuals(h, c.point, c.target, keep, **kw)
    point, target = c.point[keep != 0], c.target[keep != 0]
    out["removed"] = h
    for k, (tag, flags) in enumerate(wfc.keep_patterns(len(point), 5).items()):
        out["pattern_" + tag] = impl.remove_residuals(h, point, target, flags, **kw)
    # the points of frame 1 leave, then frame 1 itself, then the new keyframe F - 1 gets its residuals (frame F - 2 after the removal)
    keep_p = (c.host != 1).astype(np.int32)
    h = impl.remove_points(h, point, keep_p)
    host = c.host[keep_p != 0]
    new_index = np.cumsum(keep_p) - 1
    sel = keep_p[point] != 0
    point, target = new_index[point[sel]].astype(np.int32), target[sel]
    out["points_removed"] = h
    h = impl.marginalize_frame(h, point, target, 1, **kw)
    host, point, target = np.where(host > 1, host - 1, host).astype(np.int32), point[target != 1], target[target != 1]
    target = np.where(target > 1, target - 1, target).astype(np.int32)
    out["frame_removed"] = h
    for frame in (c.F - 2, 0):
        point, target, new_map, h = impl.insert_frame_residuals(h, host, point, target, frame, **kw)
        out["inserted_%d" % frame] = (point, target, new_map, h)
    masks = np.arange(40, dtype=np.uint64) * np.uint64(37) % np.uint64(1 << c.F)
    out["activated"] = impl.activated(None, masks, c.F, **kw)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_oracle_bit_for_bit(name):
    bad = _diff(_sequence(name, oracle), _sequence(name, wfh))
    assert not bad, bad[:12]


def test_defaults_and_rel_baseline():
    assert not _diff(oracle.defaults(7, 11), wfh.defaults(7, 11)) and not _diff(oracle.defaults(0, 0), wfh.defaults(0, 0))
    c = wfc.case("f8_1100")
    rng = np.random.default_rng(3)
    values = []
    for _ in range(300):
        p = int(rng.integers(0, len(c.host)))
        pc = c.precalc[int(rng.integers(0, c.F * c.F))]
        a, b = oracle.rel_baseline(pc, c.uv[p, 0], c.uv[p, 1], c.ids[p]), wfh.rel_baseline(pc, c.uv[p, 0], c.uv[p, 1], c.ids[p])
        assert wsh.same_bits(a, b)
        values.append(a)
    assert np.isfinite(values).all() and max(values) > 0.01
    # a NaN never wins, and a point that projects to infinity gives one
    pc = c.precalc[1].copy()
    pc[6:9] = 0
    assert np.isnan(oracle.rel_baseline(pc, 3.0, 4.0, 0.0)) and np.isnan(wfh.rel_baseline(pc, 3.0, 4.0, 0.0))
    h = oracle.defaults(1, 1)
    args = (np.zeros(1, np.int32), np.array([[3.0, 4.0]], np.float32), np.zeros(1, np.float32), np.zeros(1, np.int32), np.ones(1, np.int32), np.zeros(1, np.int32),
            np.ones(1, np.int32), np.tile(pc, (4, 1)), 2)
    for impl in (oracle, wfh):
        got = impl.apply_fixed(h, *args, 0)[0]
        assert got["max_rel_baseline"][0] == 0 and got["num_good"][0] == 1


def test_the_case_set_reaches_every_branch():
    """over the case set the oracle alone sees each of these at least once"""
    total = {}
    for name in NAMES:
        c = wfc.case(name)
        _, counts, seen = oracle.apply_fixed(c.history, c.host, c.uv, c.ids, c.point, c.target, c.state, c.active, c.precalc, c.F, 0)
        assert counts.sum() == len(c.point) and (counts > 0).all()
        for k, v in seen.items():
            total[k] = total.get(k, 0) + v
        lt = c.history["last_target"]
        total["same_twice"] = total.get("same_twice", 0) + int(((lt[:, 0] == lt[:, 1]) & (lt[:, 0] >= 0)).sum())
    for k in ("hit0", "hit1", "miss", "raised", "not_raised", "good", "skipped_old", "skipped_inactive", "same_twice"):
        assert total[k] > 0, k
    seq = _sequence("f8_1100", oracle)
    before, after = seq["clear_flags"][0]["last_target"], seq["removed"]["last_target"]
    assert ((before >= 0) & (after == -1)).any() and ((before >= 0) & (after == before)).any()                 # a removal forgets some, keeps others
    before, after = seq["points_removed"]["last_target"], seq["frame_removed"]["last_target"]
    assert (after == before - 1).any() and ((before == 1) & (after == -1)).any() and ((before == 0) & (after == 0)).any()
    for key in ("inserted_6", "inserted_0"):
        point, target, new_map, h = seq[key]
        assert (new_map < 0).any() and (new_map >= 0).any() and (h["is_new"][new_map < 0] == 1).all()
    a = seq["activated"]
    assert (a["last_target"][:, 0] == 7).any() and (a["last_target"][:, 0] == -1).any() and (a["last_target"][:, 1] == 6).any()
    big = wfc.case(wfc.wec.BIG)
    assert len(big.host) > 4 * 1024 and len(big.point) > 16 * 1024


def test_an_insert_is_a_stable_edit_and_a_refusal_changes_nothing():
    for name in NAMES:
        c = wfc.case(name)
        for frame in range(c.F):
            point, target, new_map, h = wfh.insert_frame_residuals(c.history, c.host, c.point, c.target, frame)
            old = new_map >= 0
            assert (new_map[old] == np.arange(len(c.point))).all()                                     # every old row, in order
            assert (point[1:] >= point[:-1]).all() and wsh.same_bits(target[old], c.target) and wsh.same_bits(h["is_new"][old], c.history["is_new"])
            new_p = point[~old]
            assert (c.host[new_p] != frame).all() and (target[~old] == frame).all()
            ends = np.searchsorted(point, new_p, side="right") - 1
            assert (ends == np.flatnonzero(~old)).all()                                                # at the END of the point's run
            for p in range(len(c.host)):                                                                # one residual per (point, target)
                t = target[np.searchsorted(point, p):np.searchsorted(point, p, side="right")]
                assert len(set(t.tolist())) == len(t) and (frame in t) == (c.host[p] != frame)
            K = int((~old).sum())
            if K:
                assert wfh.insert_frame_residuals(c.history, c.host, c.point, c.target, frame, capacity=len(c.point) + K - 1) is None
            again = wfh.insert_frame_residuals(h, c.host, point, target, frame)
            assert len(again[0]) == len(point) and not _diff(again[3], h)                              # nothing left to insert


def test_an_edited_history_behaves_as_one_set_afresh():
    """the pass over tables and history that went through the edits equals the pass over the oracle's tables with the oracle's history"""
    for name in ("f3_513", "f8_1100"):
        c = wfc.case(name)
        seq_h, seq_o = _sequence(name, wfh), _sequence(name, oracle)
        key = "inserted_0"
        host = np.where(c.host[c.host != 1] > 1, c.host[c.host != 1] - 1, c.host[c.host != 1]).astype(np.int32)
        uv, ids = c.uv[c.host != 1], c.ids[c.host != 1]
        F = c.F - 1
        keep = [f for f in range(c.F) if f != 1]
        precalc = c.precalc.reshape(c.F, c.F, 27)[np.ix_(keep, keep)].reshape(-1, 27)
        results = []
        for point, target, _, h in (seq_h[key], seq_o[key]):
            rng = np.random.default_rng(8)
            state = rng.integers(0, 3, len(point)).astype(np.int32)
            active = (state == 0).astype(np.int32)
            results.append([impl.apply_fixed(h, host, uv, ids, point, target, state, active, precalc, F, 1)[:2] for impl in (wfh, oracle)])
        assert not _diff(results[0][0], results[1][1]) and not _diff(results[0][1], results[1][0])
        assert (results[0][0][0]["num_good"] > seq_h[key][3]["num_good"]).any()


@pytest.mark.parametrize("mutate", oracle.MUTATIONS)
def test_every_mutation_of_the_oracle_is_caught(mutate):
    caught = []
    for name in NAMES[:3]:
        try:
            bad = _diff(_sequence(name, oracle, mutate), _sequence(name, wfh))
        except (IndexError, ValueError, AssertionError):             # a mutation may leave an index outside its table
            bad = ["raised"]
        if bad:
            caught.append(name)
    assert caught, mutate


# ---- flagPointsForRemoval: the decisions ----------------------------------------------------------------------------------------------------

def _flag_runs(impl, mutate=None):
    """every flag case under every mask, and removeOutliers' point loop: fates, counts and candidates"""
    kw = {} if mutate is None else dict(mutate=mutate)
    out = {}
    for F, n, seed in wfc.FLAG_CASES:
        c = wfc.flag_case(F, n, seed)
        for mask in c.masks:
            for only_empty in (False, True):
                out[(F, n, mask, only_empty)] = impl.flag_points(c.history, c.host, c.ids, c.point, c.target, c.state, c.hessian, mask, only_empty, **kw)[:3]
    for name in ("f3_513", "f8_1100"):                              # ... and on the windows of the other tests, with their histories
        c = wfc.case(name)
        hess = np.random.default_rng(6).choice([0.0, 50.0, 70.0, 1e4], len(c.host)).astype(np.float32)
        out[name] = impl.flag_points(c.history, c.host, c.ids, c.point, c.target, c.state, hess, 1 << (c.F - 1), False, **kw)[:3]
    return {str(k): v for k, v in out.items()}


def test_the_flags_of_the_restatement_equal_the_oracle():
    bad = _diff(_flag_runs(oracle), _flag_runs(wfh))
    assert not bad, bad[:12]


def test_the_flag_cases_reach_every_branch():
    """the oracle alone puts at least one point into each branch; a degenerate case set fails here"""
    total = {}
    for F, n, seed in wfc.FLAG_CASES:
        c = wfc.flag_case(F, n, seed)
        for mask in c.masks:
            fates, counts, cand, seen = oracle.flag_points(c.history, c.host, c.ids, c.point, c.target, c.state, c.hessian, mask)
            assert counts[:3].sum() == n and (counts[3:].reshape(8, 3).sum(axis=0) == counts[:3]).all()
            for k, v in seen.items():
                total[k] = total.get(k, 0) + v
            total["kept"] = total.get("kept", 0) + int(counts[0])
        only = oracle.flag_points(c.history, c.host, c.ids, c.point, c.target, c.state, c.hessian, c.masks[-1], True)[0]
        sizes = np.diff(oracle.runs(c.point, n))
        assert ((only == oracle.DROP) == (sizes == 0)).all() and (only != oracle.MARGINALIZE).all() and (sizes == 0).any()
    for k in ("negative_idepth", "empty_run", "oob_true_few_left", "oob_true_last_oob", "oob_true_two_outliers", "oob_false_short", "oob_false",
              "host_flagged_not_oob", "not_inlier", "hessian_at_or_below", "hessian_above", "kept"):
        assert total.get(k, 0) > 0, k


@pytest.mark.parametrize("mutate", oracle.FLAG_MUTATIONS)
def test_every_mutation_of_the_flagging_oracle_is_caught(mutate):
    assert _diff(_flag_runs(oracle, mutate), _flag_runs(wfh)), mutate
