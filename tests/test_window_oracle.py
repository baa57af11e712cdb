"""csrc/eds_window.hpp under g++ (tests/window_harness.py) against the numpy oracle written from the reference text
(tests/np_window_oracle.py): bit for bit on every per-residual and every per-point output, the energy within the derived bound of the
exact sum of the same fp32 terms; the cases reach every branch and leave no residual undecided on the oracle alone; and the oracle's
mutations — fx used for fy, JabJIdx(0,1) / (1,0) exchanged, the sqrtf(hw) dropped, the tap sums added in reverse pattern order — each
change at least one case (no GPU needed: nothing here launches anything)."""
import functools

import numpy as np
import pytest

import np_window_oracle as no
import window_cases as wc
import window_harness as wh

NAMES = list(wc.cases())


def oracle_case(c, **variant):
    o = no.Oracle(c.H, c.W, c.K, c.prm, **variant)
    o.set_frames(0, c.images)
    o.set_points(c.host, c.uv, c.color, c.weights, c.ids, c.idz)
    o.set_residuals(c.point, c.target, c.state, c.energy)
    return o


def oracle_rounds(c, **variant):
    """tests/window_harness.run_rounds on the oracle, with what only the oracle knows (exact energy, margins, branch counts)"""
    o, out = oracle_case(c, **variant), []
    for rnd in range(2):
        if rnd == 1:
            o.set_idepths(c.ids2)
        q = o.linearize(c.F, c.precalc, c.th)
        lin = o.residuals()
        o.apply(True)
        nres = o.point_hessians(c.prior, c.delta, c.lf, bool(c.shift))
        out.append(dict(q=q, margins=dict(o.margins), clamped=o.clamped, nres=nres, linearized=lin, residuals=o.residuals(), points=o.points()))
    return out


@functools.lru_cache(maxsize=None)
def _both(name):
    c = wc.cases()[name]
    w = wh.open_case(c)
    got = wh.run_rounds(w, c)
    frames = [w.frame(f) for f in range(c.F)]
    w.close()
    return c, got, oracle_rounds(c), frames


@pytest.mark.parametrize("name", NAMES)
def test_every_residual_and_point_output_equals_the_oracle_bit_for_bit(name):
    c, got, want, frames = _both(name)
    o = oracle_case(c)
    for f in range(c.F):
        assert no.same_bits(frames[f], o.frame(f)), (name, f)
    for rnd in range(2):
        g, w = got[rnd], want[rnd]
        for stage in ("linearized", "residuals"):
            for k, _, _ in wh.RESIDUAL_FIELDS:
                assert no.same_bits(g[stage][k], w[stage][k]), (name, rnd, stage, k)
        for k, _, _ in wh.POINT_FIELDS:
            assert no.same_bits(g["points"][k], w["points"][k]), (name, rnd, k)
        assert np.array_equal(g["counts"], w["q"]["counts"]) and g["nres"] == w["nres"]
        # the energy: every term is the oracle's bit for bit, so the fp64 fold is within n 2^-53 sum|term| of the exact sum
        m = len(c.point)
        bound = m * 2.0 ** -53 * w["q"]["abs"]
        print(f"{name}[{rnd}]: energy {g['energy']!r} exact {w['q']['energy']!r} bound {bound:.3g}")
        assert abs(g["energy"] - w["q"]["energy"]) <= bound


def test_the_cases_reach_every_branch_and_leave_no_residual_undecided():
    total, clamped, no_active, shifts, modes = {}, 0, 0, set(), set()
    for name in NAMES:
        c, _, want, _ = _both(name)
        shifts.add(bool(c.shift))
        modes.add(float(c.prm.get("affine_opt_mode_a", 1e12)) < 0)
        for rnd in range(2):
            assert want[rnd]["q"]["undecided"] == 0, (name, rnd)
            for k, v in want[rnd]["margins"].items():
                total[k] = total.get(k, 0) + v
            clamped += want[rnd]["clamped"]
            no_active += int((want[rnd]["points"]["nres"] == 0).sum())
    print(total, clamped, no_active)
    for k in ("oob_entry", "oob_drescale", "oob_centre", "oob_taps", "oob_nonfinite", "outlier_by_energy", "outlier_by_gradient", "new_in",
              "huber_quadratic", "huber_linear"):
        assert total[k] > 0, k
    assert clamped > 0 and no_active > 0 and shifts == {False, True} and modes == {False, True}
    c = wc.cases()["f8_1100"]
    pairs = set(zip(c.host[c.point].tolist(), c.target.tolist()))
    assert (c.F - 1, 0) not in pairs and len(pairs) == c.F * (c.F - 1) - 1            # one (host, target) pair has no residual at all
    assert np.bincount(c.host)[0] == 1100 and np.bincount(wc.cases()["f3_513"].host)[0] == 513 and len(wc.cases()["f2_single"].point) == 1


@pytest.mark.parametrize("variant", ["fy_is_fx", "swap_jabjidx", "no_sqrt", "reverse_taps"])
def test_a_mutated_oracle_differs_from_the_header_on_some_case(variant):
    """counts of the cases (of 4) on which the mutation changes an output are printed; DESIGN 17 states them"""
    changed = []
    for name in NAMES:
        c, got, _, _ = _both(name)
        mut = oracle_rounds(c, **{variant: True})
        same = all(no.same_bits(got[r][st][k], mut[r][st][k]) for r in range(2) for st in ("linearized", "residuals") for k, _, _ in wh.RESIDUAL_FIELDS)
        same = same and all(no.same_bits(got[r]["points"][k], mut[r]["points"][k]) for r in range(2) for k, _, _ in wh.POINT_FIELDS)
        if not same:
            changed.append(name)
    print(f"{variant}: changes {len(changed)} of {len(NAMES)} cases: {changed}")
    assert changed


def test_an_oob_linearize_leaves_j_and_the_new_energy_as_they_were():
    """the behaviour the header DEFINES where the reference leaves J half-written: a second linearize that ends OOB changes nothing of J"""
    c = wc.cases()["f3_513"]
    w = wh.open_case(c)
    w.linearize(c.F, c.precalc, c.th)
    first = w.residuals()
    w.set_idepths(idepth_zero_scaled=np.full(len(c.host), np.nan, np.float32))       # every centre projection now fails
    _, counts = w.linearize(c.F, c.precalc, c.th)
    second = w.residuals()
    assert counts[1] == len(c.point)
    for k in ("J", "new_energy", "center_projected_to", "projected_to", "energy", "state"):
        assert no.same_bits(first[k], second[k]), k
    assert (second["new_energy_with_outlier"] == -1).all() and no.same_bits(second["linearize_return"], second["energy"])
    w.close()


def test_apply_without_copy_moves_the_state_only():
    c = wc.cases()["f3_5"]
    w = wh.open_case(c)
    w.linearize(c.F, c.precalc, c.th)
    lin = w.residuals()
    w.apply(False)
    r = w.residuals()
    assert np.array_equal(r["state"], lin["new_state"]) and no.same_bits(r["energy"], lin["new_energy"])
    assert not r["is_active"].any() and not r["ef_J"].any() and not r["JpJdF"].any()
    w.close()


def test_points_without_residuals_add_nothing():
    """set_points empties the residual table: point_hessians straight after it, also after an earlier table with active residuals"""
    small, big = wc.cases()["f3_5"], wc.cases()["f3_513"]
    h = wh.open_case(small)
    h.linearize(small.F, small.precalc, small.th)
    h.apply(True)
    assert h.point_hessians(small.prior, small.delta, small.lf, True) > 0
    h.set_points(big.host, big.uv, big.color, big.weights, big.ids, big.idz)
    assert h.point_hessians(big.prior, big.delta, big.lf, False) == 0
    p = h.points()
    assert not p["nres"].any() and not p["HdiF"].any() and not p["bdSumF"].any() and not p["idepth_hessian"].any()
    h.close()


# ---- the accumulators and the stitches ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _accumulated(name):
    c = wc.cases()[name]
    w, o = wh.open_case(c), oracle_case(c)
    got = wh.run_rounds(w, c, accumulate=True)[1]["accumulated"]
    w.close()
    for rnd in range(2):
        if rnd == 1:
            o.set_idepths(c.ids2)
        o.linearize(c.F, c.precalc, c.th)
        o.apply(True)
        o.point_hessians(c.prior, c.delta, c.lf, bool(c.shift))
    return c, got, o


@pytest.mark.parametrize("name", NAMES)
def test_accumulators_and_stitched_matrices_are_within_the_derived_bounds(name):
    """every accumulator word within n 2^-53 sum|term| of the exact sum of the oracle's fp32 terms (the count words exactly); H_A, b_A,
    H_sc, b_sc within the product bound plus the propagated accumulator bound"""
    c, got, o = _accumulated(name)
    acc, bound = no.accumulate(o, c.F, c.lf)
    err = np.abs(got["acc"] - acc)
    worst = int(np.argmax(err - bound))
    print(f"{name}: {len(acc)} words, worst |err| - bound {err[worst] - bound[worst]:.3g} at word {worst}; nonzero words {(acc != 0).sum()}")
    assert (err <= bound).all(), (worst, got["acc"][worst], acc[worst], bound[worst])
    e, d, cc, _ = no.acc_offsets(c.F)
    assert np.array_equal(got["acc"][91:e:no.TOP_WORDS], acc[91:e:no.TOP_WORDS]) and np.array_equal(got["acc"][d + 64:cc:no.D_WORDS], acc[d + 64:cc:no.D_WORDS])
    want = no.stitch(c.F, acc, c.adH, c.adT)
    bounds = no.stitch_bound(c.F, acc, bound, c.adH, c.adT)
    stated = no.stitch_bound(c.F, acc, bound, c.adH, c.adT, issue=True)          # gamma_24 (|A||M||B|) + propagated, asserted as well
    for k, w_, b_, s_ in zip(("H_A", "b_A", "H_sc", "b_sc"), want, bounds, stated):
        diff = np.abs(got[k] - w_)
        print(f"  {k}: max |diff| {diff.max():.3g}, max |value| {np.abs(w_).max():.3g}, largest diff / bound {np.max(diff / np.maximum(b_, 1e-300)):.3g}")
        assert (diff <= b_).all(), k
        print(f"  {k}: largest diff / gamma_24 bound {np.max(diff / np.maximum(s_, 1e-300)):.3g}")
        assert (diff <= s_).all(), k
    assert got["nres"] == int(o.r["is_active"].sum())


def test_the_swapped_accumulator_index_changes_the_asymmetric_window():
    """h F + t for h + F t: the window is asymmetric ((7, 0) has no residual, (0, 7) has), so the mutation moves words"""
    changed = []
    for name in NAMES:
        c, got, o = _accumulated(name)
        acc, bound = no.accumulate(o, c.F, c.lf, swap_index=True)
        if not (np.abs(got["acc"] - acc) <= bound).all():
            changed.append(name)
    print(f"swap_index: changes {len(changed)} of {len(NAMES)} cases: {changed}")
    assert changed


def test_the_stages_sliced_over_a_pool_equal_the_one_thread_calls():
    """points sliced by 50 over 16 threads, the energy folded afterwards in the header's order: every output bit for bit"""
    from concurrent.futures import ThreadPoolExecutor
    c = wc.cases()["f8_1100"]
    a, b = wh.open_case(c), wh.open_case(c)
    with ThreadPoolExecutor(16) as pool:
        for rnd in range(2):
            for w in (a, b):
                w.set_idepths(c.ids2 if rnd else c.ids)
            e1, c1 = a.linearize(c.F, c.precalc, c.th)
            e2, c2 = b.linearize_pool(pool, c.F, c.precalc, c.th)
            assert e1 == e2 and np.array_equal(c1, c2)
            a.apply(True)
            b.apply_pool(pool, True)
            assert a.point_hessians(c.prior, c.delta, c.lf, True) == b.point_hessians_pool(pool, c.prior, c.delta, c.lf, True)
            ra, rb, pa, pb = a.residuals(), b.residuals(), a.points(), b.points()
            assert all(no.same_bits(ra[k], rb[k]) for k in ra) and all(no.same_bits(pa[k], pb[k]) for k in pa)
    a.close()
    b.close()


@pytest.mark.parametrize("name", NAMES)
def test_the_entry_wise_stitch_equals_the_block_wise_one_bit_for_bit(name):
    """edswin::stitch_entry (one output entry at a time, what the device's stitch kernel runs) against edswin::stitch_serial"""
    c, got, _ = _accumulated(name)
    for e, k in zip(wh.stitch_entries(c.F, got["acc"], c.adH, c.adT), ("H_A", "b_A", "H_sc", "b_sc")):
        assert no.same_bits(e, got[k]) and np.array_equal(e.view("u8"), got[k].view("u8")), k
