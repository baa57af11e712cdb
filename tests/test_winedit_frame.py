"""eds_wed_marginalize_frame and eds_wed_set_state of csrc/eds_winedit.hpp under g++ (tests/winedit_harness.py), no GPU needed.
The tables against the numpy oracle (frame 0, a middle frame and the last, F = 3 and F = 8); HM', bM' bit for bit against a numpy
restatement of the header's nine steps; within the componentwise bound of DESIGN 21 of a numpy.longdouble Schur complement; the
solve of the marginalised system against the kept components of the full system's; exact symmetry; the refusals; the mutations."""
import functools

import numpy as np
import pytest

import np_winedit_oracle as oracle
import winedit_cases as wec
import winedit_harness as weh
import winsolve_cases as wsc
import winsolve_harness as wsh

NAMES = ["f3_5", "f3_513", "f8_1100"]
CASES = [(name, f) for name in NAMES for f in wec.frames_of(wsc.cases()[name].F)]


def _diff(a, b):
    fa, fb = dict(wsh.flatten(a)), dict(wsh.flatten(b))
    assert fa.keys() == fb.keys(), sorted(set(fa) ^ set(fb))
    return [k for k in fa if not wsh.same_bits(fa[k], fb[k])]


@functools.lru_cache(maxsize=None)
def _run(name, frame):
    s = wec.cases()[name]
    w, sv = wsh.open_case(s)
    out = weh.run_frame(w, sv, weh.HostEdit(w), s, frame, wec.reduce_case)
    sv.close()
    w.close()
    return out


def _inputs(name, frame):
    s = wec.cases()[name]
    return s.HM, s.bM, s.prior[frame], s.delta_prior[frame]


@pytest.mark.parametrize("name,frame", CASES)
def test_the_tables_after_a_frame_left_equal_the_oracles(name, frame):
    s = wec.cases()[name]
    out = _run(name, frame)
    assert not (out["before"]["rows"]["host"] == frame).any() and (out["before"]["rows"]["target"] == frame).any()
    want = oracle.after_set_state(oracle.edit(out["before"], frame=frame), 1.0)
    bad = _diff(want, out["after"])
    assert not bad, bad[:12]
    assert out["after"]["state"]["is_linearized"].any() == out["before"]["state"]["is_linearized"][out["before"]["rows"]["target"] != frame].any()
    keep = [f for f in range(s.F) if f != frame]
    assert wsh.same_bits(out["frames"], out["frames_before"][keep])
    assert out["after"]["rows"]["host"].max(initial=-1) < s.F - 1 and out["after"]["rows"]["target"].max(initial=-1) < s.F - 1
    assert np.isfinite(out["next"]["solve"]["x"]).all() and len(out["next"]["solve"]["x"]) == s.N - 8


@pytest.mark.parametrize("name,frame", CASES)
def test_the_arithmetic_equals_the_numpy_restatement_bit_for_bit(name, frame):
    HM, bM, prior, dp = _inputs(name, frame)
    out = _run(name, frame)
    want = oracle.marginalize_frame(HM, bM, frame, prior, dp)
    assert wsh.same_bits(want[0], out["HM"]) and wsh.same_bits(want[1], out["bM"])
    rc, h2, b2 = weh.marg_arith(frame, prior, dp, HM, bM)
    assert rc == wsh.OK and wsh.same_bits(h2, out["HM"]) and wsh.same_bits(b2, out["bM"])
    assert (out["HM"] == out["HM"].T).all()                      # 0.5 * (T + T^T) is exactly symmetric


def test_the_stated_inverse_pivots_and_refuses():
    rng = np.random.default_rng(3)
    for _ in range(20):
        a = rng.standard_normal((8, 8))
        a[rng.integers(0, 8)] *= 1e6                             # rows change places
        rc, hpi = weh.inverse8(a)
        assert rc == wsh.OK and wsh.same_bits(hpi, oracle.inverse8(a))
        assert np.abs(hpi @ a - np.eye(8)).max() < 1e-9
    tie = np.eye(8)
    tie[1, 0] = tie[3, 0] = -1.0                                 # |a_00| = |a_10| = |a_30|: the lowest row stays the pivot
    assert wsh.same_bits(weh.inverse8(tie)[1], oracle.inverse8(tie))
    singular = np.ones((8, 8))
    assert weh.inverse8(singular)[0] == wsh.NOT_USABLE and oracle.inverse8(singular) is None
    assert weh.inverse8(np.zeros((8, 8)))[0] == wsh.NOT_USABLE


@pytest.mark.parametrize("name,frame", CASES)
def test_the_result_meets_its_bound_and_the_full_systems_solve(name, frame, capsys):
    HM, bM, prior, dp = _inputs(name, frame)
    out = _run(name, frame)
    Hx, bx, Sh, A, W, bh, wb, cond = oracle.marginalize_frame_extended(HM, bM, frame, prior, dp)
    bound_H, bound_b = oracle.frame_bound(Sh, A, W, bh, wb, cond)
    err_H = np.abs(out["HM"].astype(np.longdouble) - Hx).astype(np.float64)
    err_b = np.abs(out["bM"].astype(np.longdouble) - bx).astype(np.float64)
    used_H, used_b = float((err_H / bound_H).max()), float((err_b / bound_b).max())
    norm_H = float(np.linalg.norm(err_H) / np.linalg.norm(bound_H))
    # the property that needs no restatement: solving the marginalised system gives the kept components of the full system's solve
    N = len(bM)
    P = oracle.permutation(N, frame)
    full, bfull = np.asarray(HM)[np.ix_(P, P)].copy(), np.asarray(bM)[P].copy()
    full[np.arange(N - 8, N), np.arange(N - 8, N)] += prior
    bfull[N - 8:] += prior * dp
    x_full = np.linalg.solve(full, bfull)[:N - 8]
    x_marg = np.linalg.solve(out["HM"], out["bM"])
    rel = float(np.linalg.norm(x_full - x_marg) / np.linalg.norm(x_full))
    tol = float(np.linalg.cond(full)) * N * 2.0 ** -53
    with capsys.disabled():
        print(f"\n{name} frame {frame}: cond of the scaled 8 x 8 {cond:.3f}; fraction of the componentwise bound used: HM' {used_H:.4f}, bM' {used_b:.4f}; "
              f"normwise HM' {norm_H:.4f}; solve: relative difference {rel:.3e} of the allowed {tol:.3e}")
    assert used_H <= 1.0 and used_b <= 1.0 and norm_H <= 1.0
    assert rel <= tol


def test_a_zero_block_without_a_prior_is_not_usable_and_nothing_changes():
    s = wec.cases()["f3_513"]
    frame = 1
    w, sv = wsh.open_case(s)
    ed = weh.HostEdit(w)
    weh.prepare(w, sv, s)
    ed.remove_points((ed.rows()["host"] == frame).astype(np.int32))
    before = weh.snapshot(w, sv, ed)
    HM, bM = s.HM.copy(), s.bM.copy()
    io = 4 + 8 * frame
    HM[io:io + 8, :] = 0
    HM[:, io:io + 8] = 0
    zero = np.zeros(8)
    with pytest.raises(wsh.HostError) as e:
        ed.marginalize_frame(frame, zero, zero, HM, bM)
    assert e.value.code == wsh.NOT_USABLE and oracle.marginalize_frame(HM, bM, frame, zero, zero) is None
    h2, b2 = HM.copy(), bM.copy()
    assert weh.marg_arith(frame, zero, zero, h2, b2)[0] == wsh.NOT_USABLE and wsh.same_bits(h2, HM) and wsh.same_bits(b2, bM)
    assert not _diff(before, weh.snapshot(w, sv, ed))
    # with the prior the same block is usable
    assert weh.marg_arith(frame, s.prior[frame], s.delta_prior[frame], HM, bM)[0] == wsh.OK
    sv.close()
    w.close()


def test_the_refusals_change_nothing():
    s = wec.cases()["f3_513"]
    w, sv = wsh.open_case(s)
    ed = weh.HostEdit(w)
    with pytest.raises(wsh.HostError) as e:                      # no state yet
        ed.marginalize_frame(1, s.prior[1], s.delta_prior[1], s.HM, s.bM)
    assert e.value.code == wsh.STATE
    weh.prepare(w, sv, s)
    before = weh.snapshot(w, sv, ed)
    bad = s.HM.copy()
    bad[2, 3] = np.inf
    for code, call in ((wsh.STATE, lambda: ed.marginalize_frame(0, s.prior[0], s.delta_prior[0], s.HM, s.bM)),          # frame 0 hosts points
                       (wsh.INVALID, lambda: ed.marginalize_frame(3, s.prior[0], s.delta_prior[0], s.HM, s.bM)),
                       (wsh.INVALID, lambda: ed.marginalize_frame(-1, s.prior[0], s.delta_prior[0], s.HM, s.bM)),
                       (wsh.INVALID, lambda: ed.marginalize_frame(1, s.prior[1], s.delta_prior[1], bad, s.bM)),
                       (wsh.INVALID, lambda: ed.marginalize_frame(1, s.prior[1] * np.nan, s.delta_prior[1], s.HM, s.bM)),
                       (wsh.INVALID, lambda: ed.marginalize_frame(1, s.prior[1], s.delta_prior[1], s.HM, np.full_like(s.bM, np.inf)))):
        with pytest.raises(wsh.HostError) as e:
            call()
        assert e.value.code == code
        assert not _diff(before, weh.snapshot(w, sv, ed))
    # F = 2 is refused: a window of two frames marginalises none
    s2 = wec.cases()["f2_single"]
    w2, sv2 = wsh.open_case(s2)
    ed2 = weh.HostEdit(w2)
    weh.prepare(w2, sv2, s2)
    ed2.remove_points(np.ones(w2.n, np.int32))
    with pytest.raises(wsh.HostError) as e:
        ed2.marginalize_frame(0, s2.prior[0], s2.delta_prior[0], s2.HM, s2.bM)
    assert e.value.code == wsh.INVALID
    for a, b in ((sv, w), (sv2, w2)):
        a.close()
        b.close()


def test_set_state_from_the_device_rows_equals_set_state_from_the_host():
    """eds_wed_set_state on a window that never had a state gives what eds_wsv_set_state gives with priorF = 0 and setDeltaF's deltaF"""
    s = wec.cases()["f8_1100"]
    c = s.win
    w, sv = wsh.open_case(s)
    ed = weh.HostEdit(w)
    wsh.lin_apply(w, s)
    ed.set_state(s.F, c.adH, c.adT, s.delta, s.prior, s.delta_prior, s.cPrior, s.cDelta)
    a = weh.snapshot(w, sv, ed)
    w2, sv2 = wsh.open_case(s)
    ed2 = weh.HostEdit(w2)
    wsh.lin_apply(w2, s)
    sv2.set_state(s.F, c.adH, c.adT, s.delta, s.prior, s.delta_prior, s.cPrior, s.cDelta, None, c.ids - c.idz)
    assert (c.ids != c.idz).any() and not _diff(a, weh.snapshot(w2, sv2, ed2))
    # ... and on a window WITH a state it keeps priorF and the linearized residuals
    weh.prepare(w2, sv2, s)
    before = weh.snapshot(w2, sv2, ed2)
    ed2.set_state(s.F, c.adH, c.adT, s.delta, s.prior, s.delta_prior, s.cPrior, s.cDelta)
    assert before["state"]["is_linearized"].any() and before["state"]["priorF"].any()
    assert not _diff(oracle.after_set_state(before, 1.0), weh.snapshot(w2, sv2, ed2))
    for x in (sv, w, sv2, w2):
        x.close()


@pytest.mark.parametrize("mutate", oracle.FRAME_MUTATIONS)
def test_every_mutation_of_the_table_oracle_is_caught(mutate):
    caught = [c for c in CASES if _diff(oracle.after_set_state(oracle.edit(_run(*c)["before"], frame=c[1], mutate=mutate), 1.0), _run(*c)["after"])]
    assert caught, mutate


@pytest.mark.parametrize("mutate", oracle.ARITH_MUTATIONS)
def test_every_mutation_of_the_restatement_is_caught(mutate):
    caught = []
    for name, frame in CASES:
        got = oracle.marginalize_frame(*_inputs(name, frame)[:2], frame, *_inputs(name, frame)[2:], mutate=mutate)
        out = _run(name, frame)
        if got is None or not (wsh.same_bits(got[0], out["HM"]) and wsh.same_bits(got[1], out["bM"])):
            caught.append((name, frame))
    assert caught, mutate
