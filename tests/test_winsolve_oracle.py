"""csrc/eds_winsolve.hpp under g++ (tests/winsolve_harness.py) against the numpy restatement of the reference's text
(tests/np_winsolve_oracle.py), no GPU: bit for bit on adHTdeltaF, res_toZeroF, resApprox, the L sums, the Schur prologue, the assembled
system given the same stitched matrices, xAd, the steps given the same x and the stepped inverse depths; mode 1's accumulator words and
both energies within n 2^-53 sum|term| of math.fsum; H_L / b_L and through them the assembled system within the stitch bound of DESIGN
17 plus one rounding per addition; the solve within its componentwise backward bound and, normwise, within that bound times the
condition number of numpy.linalg.solve's answer; mode 0's sums and top words under the linearized flags and the whole point
marginalisation against the oracle; no undecided comparison; and ten mutations of the oracle each change some case."""
import functools
import math

import numpy as np
import pytest

import np_window_oracle as no
import np_winsolve_oracle as nw
import winsolve_cases as wsc
import winsolve_harness as wsh

NAMES = list(wsc.ROUNDS)
U = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def run(name):
    """the host's sequence once per case, with the residual table and the raw stitches at every solve"""
    s = wsc.cases()[name]
    w, sv = wsh.open_case(s)
    seen = {}

    def probe(tag, w_, sv_):
        seen[tag] = dict(residuals=w_.residuals(), raw=sv_.raw(), l_points=sv_.l_energy_points(), points=w_.points(), state=sv_.get(system=False))

    out = wsh.run_sequence(w, sv, s, probe)
    sv.close()
    w.close()
    return s, out, seen


def tables(name, k):
    s, out, seen = run(name)
    rec = out[1 + k]
    return s, rec, seen[f"round{k}"], nw.Tables(s, seen[f"round{k}"]["residuals"], rec["state"]["is_linearized"])


def bits(a, b):
    return wsh.same_bits(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("name", NAMES)
def test_per_residual_and_per_point_outputs_equal_the_oracle_bit_for_bit(name):
    s, out, seen = run(name)
    c = s.win
    adht = nw.adht_delta(s.F, c.adH, c.adT, s.delta)
    assert bits(adht, out[0]["state"]["adHTdeltaF"])
    undecided = 0
    for k, r in enumerate(s.rounds):
        s, rec, sn, T = tables(name, k)
        st, pts = rec["state"], rec["points"]
        if k == 0:                                              # fixLinearizationF ran on this table
            rtz = nw.fix_linearization(T, adht)
            assert bits(rtz[s.fix != 0], st["res_toZeroF"][s.fix != 0]) and not st["res_toZeroF"][s.fix == 0].any()
            assert np.array_equal(st["is_linearized"] != 0, s.fix != 0)
        approx = nw.res_approx(T, adht, st["res_toZeroF"])
        assert bits(approx[T.lin], st["resApprox"][T.lin])
        lf = nw.lf_sums(T, st["resApprox"], T.lin & T.active)
        assert bits(lf, st["lf"])
        assert rec["solve"]["res_in_l"] == int((T.lin & T.active).sum()) and rec["solve"]["res_in_a"] == int((~T.lin & T.active).sum())
        a0, _ = nw.mode0_sums(T)                                # addPoint<0> skips what is linearized
        assert bits(a0[:, 0], pts["Hdd_accAF"]) and bits(a0[:, 1], pts["bd_accAF"]) and bits(a0[:, 2:], pts["Hcd_accAF"])
        hdi, bds, und = nw.schur_prologue(T, pts, lf, shift=True)
        undecided += und
        assert bits(hdi, pts["HdiF"]) and bits(bds, pts["bdSumF"])
        x = rec["solve"]["x"]
        xAd = nw.x_ad(s, x, c.adH, c.adT)
        assert bits(xAd, st["xAd"])
        step = nw.steps(T, pts, lf, xAd, x)
        assert bits(step, rec["steps"]) and bits(step, st["step"])
        assert bits(nw.stepped(st["idepth_scaled"], r.fac, step), rec["stepped"])
        assert bits(-x, st["frame_step"])
    assert undecided == 0
    live = out[1]["points"]["nres"] > 0
    if name != "f2_single":
        assert (~live).any() and live.any()                      # points with no active residual


def test_the_cases_cover_what_the_issue_lists():
    rounds = [r for v in wsc.ROUNDS.values() for r in v]
    assert {bool(r.mode & wsc.SYSTEM) for r in rounds} == {True, False}                  # both assembly branches
    assert {r.hff for r in rounds if r.mode & wsc.SYSTEM} == {True, False}
    assert any(r.mode & wsc.USE_GN for r in rounds) and any(r.mode & wsc.FIX_LAMBDA for r in rounds)
    assert any(not r.mode & (wsc.USE_GN | wsc.FIX_LAMBDA) and r.lam > 0 for r in rounds)  # a caller's lambda
    assert {r.iteration for r in rounds} == {0, 2} and {r.use_p for r in rounds} == {True, False} and {r.fac for r in rounds} == {1.0, 0.25}
    assert [wsc.cases()[k].N for k in NAMES] == [20, 28, 28, 68]
    for name in NAMES:
        s, out, seen = run(name)
        T = tables(name, 0)[3]
        per_point = [(T.lin[T.first[p]:T.first[p + 1]], T.active[T.first[p]:T.first[p + 1]]) for p in range(T.n)]
        all_lin = sum(1 for l, a in per_point if a.any() and l[a].all())
        assert (all_lin > 0) == (name != "f3_5"), name           # points all of whose residuals are linearized
        frac = T.lin.mean() if T.m else 0
        assert {"f2_single": frac == 1, "f3_5": frac == 0, "f3_513": 0.25 < frac < 0.5, "f8_1100": 0.2 < frac < 0.5}[name]
        assert out[1]["solve"]["orthogonalized_system"] == int(name == "f8_1100") and out[2]["solve"]["orthogonalized_x"] == 1
        assert 0 < s.marg.sum() <= max(1, 0.2 * s.n) and out[-1]["res_in_m"] > 0 or name == "f3_5"
        assert all(np.isfinite(r["solve"]["x"]).all() for r in out[1:])


@pytest.mark.parametrize("name", NAMES)
def test_accumulators_assembly_and_energies_are_within_the_derived_bounds(name):
    s, out, seen = run(name)
    c = s.win
    for k, r in enumerate(s.rounds):
        s, rec, sn, T = tables(name, k)
        st, raw = rec["state"], sn["raw"]
        # mode 1's accumulator words against the exact sums of the oracle's fp32 terms
        acc, bound = nw.top_acc_exact(T, st["resApprox"], T.lin & T.active)
        err = np.abs(raw["accL"] - acc)
        assert (err <= bound).all(), int(np.argmax(err - bound))
        # mode 0's top words under the flags: the residuals that are active and not linearized
        acc0, bound0 = nw.top_acc_exact(T, T.J[:, :8], nw.mode0_sums(T)[1])
        assert (np.abs(raw["acc"][:len(acc0)] - acc0) <= bound0).all()
        # H_L, b_L against the numpy stitch of the exact words: DESIGN 17's bound
        full, fb = np.zeros(no.acc_offsets(s.F)[3]), np.zeros(no.acc_offsets(s.F)[3])
        full[:len(acc)], fb[:len(acc)] = acc, bound
        HLx, bLx = no.stitch(s.F, full, c.adH, c.adT)[:2]
        HLb, bLb = no.stitch_bound(s.F, full, fb, c.adH, c.adT)[:2]
        assert (np.abs(raw["H_L"] - HLx) <= HLb).all() and (np.abs(raw["b_L"] - bLx) <= bLb).all()
        # the assembly: the oracle's statements on the same stitched matrices give the same bits ...
        Hf, bf, lastH, lastb = nw.assemble(s, r, raw, s.HM, s.bM)
        assert bits(Hf, st["HFinal"]) and bits(bf, st["bFinal"]) and bits(lastH, rec["solve"]["lastHS"]) and bits(lastb, rec["solve"]["lastbS"])
        # ... and on the exact H_L, b_L they stay within the stitch bound plus one rounding per addition (at most six
        # additions and two scalings touch an entry; the orthogonalised system adds its two N-term dot products per entry)
        Hx, bx, lHx, lbx = nw.assemble(s, r, dict(raw, H_L=HLx, b_L=bLx), s.HM, s.bM)
        lam = rec["solve"]["lam"]
        if rec["solve"]["orthogonalized_system"]:
            bH, bb = nw.orth_system_bound(s, raw, HLb, bLb, lam, s.HM, s.bM)
        else:
            mag = np.abs(raw["H_L"]) + np.abs(raw["H_A"]) + np.abs(raw["H_sc"]) + np.abs(s.HM) + np.diag(np.concatenate([s.cPrior, s.prior.ravel()]))
            bH = (1 + lam) * HLb + 8 * U * (1 + lam) * mag
            magb = np.abs(raw["b_L"]) + np.abs(raw["b_A"]) + np.abs(raw["b_sc"]) + np.abs(s.bM) + np.abs(s.HM) @ np.abs(nw.stitched_delta(s)) + 1.0
            bb = bLb + (s.N + 8) * U * magb
        fr = float(np.max(np.abs(Hx - st["HFinal"]) / np.maximum(bH, 1e-300)))
        fr2 = float(np.max(np.abs(lHx - rec["solve"]["lastHS"]) / np.maximum(bH, 1e-300)))
        fb_ = float(np.max(np.abs(bx - st["bFinal"]) / np.maximum(bb, 1e-300)))
        fb2 = float(np.max(np.abs(lbx - rec["solve"]["lastbS"]) / np.maximum(bb, 1e-300)))
        print(f"{name}[{k}]: assembled HFinal {fr:.3g}, lastHS {fr2:.3g}, bFinal {fb_:.3g}, lastbS {fb2:.3g} of the bound"
              f"{' (orthogonalised system)' if rec['solve']['orthogonalized_system'] else ''}")
        assert fr <= 1 and fr2 <= 1 and fb_ <= 1 and fb2 <= 1
        # the energies
        adht = st["adHTdeltaF"]
        terms = nw.l_energy_terms(T, adht, st["res_toZeroF"])
        per_point = np.array([math.fsum(t) for t in terms])
        assert (np.abs(sn["l_points"] - per_point) <= np.array([len(t) * U * math.fsum(abs(v) for v in t) for t in terms])).all()
        exact = math.fsum(v for t in terms for v in t) + nw.l_energy_priors(s)
        nterm = sum(len(t) for t in terms) + 8 * s.F + 5
        mag = math.fsum(abs(v) for t in terms for v in t) + abs(nw.l_energy_priors(s))
        print(f"{name}[{k}]: L energy {rec['l_energy']!r} exact {exact!r}, {abs(rec['l_energy'] - exact) / (nterm * U * mag):.3g} of the bound")
        assert abs(rec["l_energy"] - exact) <= nterm * U * mag
        mexact, mmag = nw.m_energy_terms(s, s.HM, s.bM)
        assert abs(rec["m_energy"] - mexact) <= (2 * s.N + 2) * U * mmag


@pytest.mark.parametrize("name", NAMES)
def test_the_solve_meets_its_backward_bound_and_numpy(name):
    s, out, seen = run(name)
    ties = 0
    for k, rec in enumerate(out[1:]):
        st = rec["state"]
        H, b = st["HFinal"], st["bFinal"]
        x0, L, d, perm = wsh.ldlt(H, b)
        orth = rec["solve"]["orthogonalized_x"]
        want = x0 - nw.rows_times(s.P, x0) if orth else x0
        assert bits(want, rec["solve"]["x"])
        S = 1.0 / np.sqrt(np.diag(H) + 10.0)
        frac, bound, t = nw.ldlt_check(H, b, x0 / S, L, d, perm)
        ties += t
        # HFinal_top is symmetric only to fp32 rounding (accD's (HdiF J1) J2 is not the transpose of (HdiF J2) J1), and an LDLT reads
        # ONE triangle, Eigen's and this one the lower: numpy gets the matrix as the solve reads it
        A = np.tril((S[:, None] * H) * S[None, :])
        A = A + np.tril(A, -1).T
        xn = np.linalg.solve(A, S * b)
        cond = np.linalg.cond(A)
        eta = np.max(bound) / (np.linalg.norm(A, np.inf) * np.max(np.abs(x0 / S)))
        second = cond * eta                                     # the backward bound times the condition number
        dist = np.linalg.norm(x0 / S - xn, np.inf) / np.linalg.norm(xn, np.inf)
        print(f"{name} {rec['tag']}: backward {frac:.3g} of the bound; cond {cond:.3g}, normwise distance {dist:.3g}, {dist / second:.3g} of {second:.3g}")
        assert frac <= 1 and dist <= second and second < 1e-3
        assert np.array_equal(np.sort(perm), np.arange(s.N))
    assert ties == 0


def test_a_zero_pivot_gives_a_zero_component():
    H = np.zeros((3, 3))                                        # row and column 1 are zero: the last pivot is exactly 0
    H[0, 0], H[2, 2], H[0, 2], H[2, 0] = 4.0, 9.0, 1.0, 1.0
    x, L, d, perm = wsh.ldlt(H, np.array([1.0, 5.0, 2.0]))
    assert d[2] == 0.0 and perm[2] == 1 and x[1] == 0.0 and np.isfinite(x).all()
    assert np.allclose(H[np.ix_([0, 2], [0, 2])] @ x[[0, 2]], [1.0, 2.0], rtol=1e-14)


@pytest.mark.parametrize("name", NAMES)
def test_the_marginalisation_equals_the_oracle(name):
    """priorF, the mode 2 sums, the Schur addPoint(p, false) bit for bit on the flagged points; every accumulator word within
    n 2^-53 sum|term| of the exact sums; M, Mb, Msc, Mbsc within DESIGN 17's stitch bound; HM, bM bit for bit from the same stitches"""
    got = _marg(name)
    s, T, sn, rec, m = got["s"], got["T"], got["sn"], got["rec"], got["m"]
    priorF, lf, hdi, bds, acc, bound = got["oracle"]
    pts, st = sn["points"], sn["state"]
    assert bits(priorF, st["priorF"]) and bits(lf[m], st["lf"][m])
    assert bits(hdi[m], pts["HdiF"][m]) and bits(bds[m], pts["bdSumF"][m])
    assert not pts["Hdd_accAF"][m].any() and not pts["bd_accAF"][m].any() and not pts["Hcd_accAF"][m].any()
    assert rec["res_in_m"] == int((T.active & m[T.point]).sum())
    assert (np.abs(sn["raw"]["acc"] - acc) <= bound).all()
    c = s.win
    want, bounds = no.stitch(s.F, acc, c.adH, c.adT), no.stitch_bound(s.F, acc, bound, c.adH, c.adT)
    for key, w_, b_ in zip(("H_A", "b_A", "H_sc", "b_sc"), want, bounds):
        assert (np.abs(sn["raw"][key] - w_) <= b_).all(), key
    HM, bM = nw.marg_update(s.HM, s.bM, sn["raw"], wsc.WEIGHT_FAC)
    assert bits(HM, rec["HM"]) and bits(bM, rec["bM"])


@functools.lru_cache(maxsize=None)
def _marg(name):
    s, out, seen = run(name)
    sn, rec = seen["marg"], out[-1]
    T = nw.Tables(s, sn["residuals"], sn["state"]["is_linearized"])
    m = s.marg != 0
    before = out[len(s.rounds)]                                  # the last round: the L sums its solve left
    oracle = nw.marginalise(T, s, sn["state"]["res_toZeroF"], before["points"], before["state"]["lf"], s.marg, wsc.PRIOR_FAC)
    return dict(s=s, T=T, sn=sn, rec=rec, m=m, oracle=oracle, before=before)


MUTATIONS = ("xAd_index", "adHostF_index", "fix_sign", "shift_flipped", "no_divisor", "prior_delta", "mode2_filter", "mode0_ignores_lin",
             "marg_shift", "marg_sign")


@pytest.mark.parametrize("mut", MUTATIONS)
def test_a_mutated_oracle_differs_from_the_header_on_some_case(mut):
    changed = []
    for name in NAMES:
        s, out, seen = run(name)
        c = s.win
        for k, r in enumerate(s.rounds):
            s, rec, sn, T = tables(name, k)
            st, pts = rec["state"], rec["points"]
            if mut == "xAd_index":
                same = bits(nw.x_ad(s, rec["solve"]["x"], c.adH, c.adT, mut), st["xAd"])
            elif mut == "adHostF_index":
                same = bits(nw.adht_delta(s.F, c.adH, c.adT, s.delta, mut), st["adHTdeltaF"])
            elif mut == "fix_sign":
                same = k > 0 or bits(nw.fix_linearization(T, st["adHTdeltaF"], mut)[s.fix != 0], st["res_toZeroF"][s.fix != 0])
            elif mut == "shift_flipped":
                same = bits(nw.schur_prologue(T, pts, st["lf"], shift=False)[1], pts["bdSumF"])
            elif mut == "mode0_ignores_lin":
                a0, take = nw.mode0_sums(T, mut)
                acc0, bound0 = nw.top_acc_exact(T, T.J[:, :8], take)
                same = bits(a0[:, 0], pts["Hdd_accAF"]) and bool((np.abs(sn["raw"]["acc"][:len(acc0)] - acc0) <= bound0).all())
            elif mut in ("marg_shift", "marg_sign"):
                if k:
                    continue
                g = _marg(name)
                if mut == "marg_shift":
                    bds = nw.marginalise(g["T"], s, g["sn"]["state"]["res_toZeroF"], g["before"]["points"], g["before"]["state"]["lf"],
                                         s.marg, wsc.PRIOR_FAC, mut)[3]
                    same = bits(bds[g["m"]], g["sn"]["points"]["bdSumF"][g["m"]])
                else:
                    HM, bM = nw.marg_update(s.HM, s.bM, g["sn"]["raw"], wsc.WEIGHT_FAC, mut)
                    same = bits(HM, g["rec"]["HM"]) and bits(bM, g["rec"]["bM"])
            elif mut == "mode2_filter":
                same = bits(nw.lf_sums(T, np.where(T.lin[:, None], st["resApprox"], T.J[:, :8]), T.active), st["lf"])
            else:
                Hf, bf, _, _ = nw.assemble(s, r, sn["raw"], s.HM, s.bM, mut)
                same = bits(Hf, st["HFinal"]) and bits(bf, st["bFinal"])
            if not same:
                changed.append((name, k))
    assert changed, mut
