"""csrc/eds_init.hpp under g++ (tests/init_harness.py, the serial evaluator that walks the device's order) against
tests/np_init_oracle.py, the numpy restatement of the reference in the reference's own loop order (no GPU needed).

Given the same pose and point state, everything per tap and per point is bit for bit, and so are the steps without a reordered sum
(doStep, applyStep, optReg, resetPoints, propagateDown, propagateUp); the sums are within n 2^-53 sum|term| of the exact sum of the
same fp32 terms; a whole sequence is within a bound MEASURED against the oracle.  The conditions the issue puts on the cases are
asserted here, so a GPU test cannot pass by never reaching the code.

Measured on the three cases, serial evaluator against the oracle over every frame: the largest difference of a pose entry 4.0e-7 (edges,
frame 6), of the affine pair 4.0e-6 (b64, frame 3); the accept sequences are identical.  The bounds below are 4 x those."""
import functools

import numpy as np
import pytest

import init_cases as ic
import init_harness as ih
import inisetup_harness as sh
import np_init_oracle as no

POSE_BOUND, AFF_BOUND = 4 * 4.0e-7, 4 * 4.0e-6
POINT_FIELDS = ih.POINT.names


@functools.lru_cache(maxsize=None)
def _host_run(name):
    """the serial evaluator over the case's sequence: per frame the points before it, the carry before it, and the result"""
    c = ic.cases()[name]
    t = ih.open_case(c)
    frames = []
    for k, f in enumerate(c.frames):
        before = [t.points(l) for l in range(c.levels)]
        jb = [t.jb(l, 0) for l in range(c.levels)]
        carry = t.carry().copy()
        r = t.trackFrame(f, c.exposures[k + 1], 1).copy()
        frames.append(dict(before=before, jb=jb, carry=carry, result=r, after=[t.points(l) for l in range(c.levels)]))
    t.close()
    return frames


def _same(a, b, fields=POINT_FIELDS, what=""):
    for f in fields:
        assert no.same_bits(a[f], b[f]), (what, f, np.nonzero(a[f] != b[f]))


def test_cases_have_the_sizes_the_issue_asks_for():
    a, b = ic.cases()["a96"], ic.cases()["b64"]
    n0 = len(a.uv[0])
    assert (a.W, a.H, a.levels) == (96, 80, 3) and 513 <= n0 <= 1023 and n0 % 64 != 0
    assert len(a.uv[2]) == (24 - 7) * (20 - 7)                                        # the top level at full density
    assert (b.W, b.H, b.levels) == (64, 48, 2) and b.prm["fix_affine"] == 0 and min(b.exposures) > 0 and len(set(b.exposures)) > 1
    e = ic.cases()["edges"]
    assert e.pose_guess is not None and any((nb == -1).any() for nb in e.nb)
    assert any(((nb != -1).sum(axis=1) <= 2).any() for nb in e.nb)
    for c in ic.cases().values():                            # the cases' tables in numpy equal edsini::make_nn_exhaustive's (any valid
        for l in range(c.levels):                            # table is an input here; tests/test_nn_pin.py holds make_nn to nanoflann)
            nb, par = sh.make_nn_exhaustive(c.uv[l], c.uv[l + 1] if l + 1 < c.levels else None)
            enb, epar = ic.exact_nn(c.uv[l], c.uv[l + 1] if l + 1 < c.levels else None)
            assert np.array_equal(nb, enb) and (par is None or np.array_equal(par, epar))


def test_a96_snaps_by_its_fourth_frame_and_is_ready_later():
    fr = _host_run("a96")
    snapped = [int(f["result"]["snapped"]) for f in fr]
    ready = [int(f["result"]["ready"]) for f in fr]
    assert snapped[0] == 0 and snapped[3] == 1
    first = snapped.index(1)
    assert 1 in ready and ready.index(1) > first and fr[first]["result"]["snapped_at"] == first + 1
    # |t| passes sqrt(alphaK / alphaW) = 0.0167 where it snaps
    assert fr[first - 1]["result"]["rescale"] < 2.5 / 150 < fr[first + 1]["result"]["rescale"]


@pytest.mark.parametrize("name", list(ic.cases()))
def test_every_case_rejects_and_accepts(name):
    acc = rej = 0
    for f in _host_run(name):
        r = f["result"]
        d = r["decisions"][:r["n_decisions"]]
        acc += int((d & 1).sum()); rej += int((1 - (d & 1)).sum())
        assert r["iterations"].sum() == r["n_decisions"] and r["accepts"].sum() == (d & 1).sum() and r["launches"] == 1 and r["waits"] == 1
    assert acc >= 1 and rej >= 1


def test_edges_has_points_going_bad_and_points_revived():
    c, fr = ic.cases()["edges"], _host_run("edges")
    top = c.levels - 1
    went_bad = sum(int((f["before"][l]["isGood"] & ~f["after"][l]["isGood"] & 1).sum()) for f in fr for l in range(c.levels))
    revived = 0
    for k, f in enumerate(fr):
        if not (f["before"][top]["isGood"] == 0).any():
            continue
        t = ih.open_case(c)
        t.set_state(top, f["before"][top])
        t.reset_points(top)
        revived += int((t.points(top)["isGood"] & ~f["before"][top]["isGood"] & 1).sum())
        t.close()
    assert went_bad >= 1 and revived >= 1, (went_bad, revived)
    # the nnn <= 2 branch: a good point of a snapped frame with at most two good neighbours keeps its iR through optReg
    nb = c.nb[top]
    assert ((nb != -1).sum(axis=1) <= 2).any()


def _bad_after_first_calc(name):
    """the points of every level that the first calcResAndGS of the first frame finds bad, at the pose the frame starts from"""
    c = ic.cases()[name]
    t = ih.open_case(c)
    t.set_new(c.frames[0])
    T = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1) if c.pose_guess is None else c.pose_guess.copy()
    T[:, 3] = 0                                                    # the un-snapped reset of :90
    bad = []
    for lvl in range(c.levels):
        t.reset_points(lvl)
        t.calc(lvl, T, (0.0, 0.0))
        P = t.points(lvl)
        bad.append((P["isGood_new"] == 0) & (P["u"] > 0.75 * (c.W >> lvl)))        # the border the guess turns towards
    t.close()
    return bad, c


def test_the_pose_guess_of_edges_pushes_a_band_of_points_out_of_the_image():
    """the guess turns the camera about y: on every level the first evaluation loses points next to the right border, which the
    same frame from the identity (a96) keeps"""
    bad_e, c = _bad_after_first_calc("edges")
    bad_a, _ = _bad_after_first_calc("a96")
    top = c.levels - 1
    for lvl in range(c.levels):
        print(f"level {lvl}: bad near the border, edges {int(bad_e[lvl].sum())} a96 {int(bad_a[lvl].sum())}")
        assert bad_e[lvl].sum() > bad_a[lvl].sum()
    assert bad_e[top].sum() >= (c.H >> top) - 7                    # a whole column of the top level's rectangle at the least


def _oracle_at(c, frame, k):
    """an oracle holding the state the serial evaluator had before frame k"""
    o = no.Oracle(c)
    o.pts = [p.copy() for p in frame["before"]]
    o.jb = [j.copy() for j in frame["jb"]]
    o.snapped = bool(frame["carry"]["snapped"])
    o.set_new(c.frames[k])
    return o


def _host_at(c, frame, k):
    t = ih.open_case(c)
    for l in range(c.levels):
        t.set_state(l, frame["before"][l], frame["jb"][l])
    t.set_new(c.frames[k])
    return t


def test_in_order_loops_differ_from_jacobi_on_the_top_level():
    """the inputs were chosen so that an optReg / resetPoints that reads only old values gives other bits: a schedule that got the
    dependencies wrong could not pass the bit-for-bit tests below"""
    c, fr = ic.cases()["a96"], _host_run("a96")
    top = c.levels - 1
    k = [int(f["carry"]["snapped"]) for f in fr].index(1)
    a, b = _oracle_at(c, fr[k], k), _oracle_at(c, fr[k], k)
    a.opt_reg(top); b.opt_reg(top, jacobi=True)
    assert not no.same_bits(a.pts[top]["iR"], b.pts[top]["iR"])
    # resetPoints on the state the sequence itself reaches: before the last frame the top level holds bad points that are neighbours,
    # so a later one sees an earlier one revived
    k = len(fr) - 1
    before = fr[k]["before"][top]
    assert (before["isGood"] == 0).sum() >= 2
    a, b = _oracle_at(c, fr[k], k), _oracle_at(c, fr[k], k)
    a.reset_points(top); b.reset_points(top, jacobi=True)
    assert ((a.pts[top]["isGood"] != 0) & (before["isGood"] == 0)).sum() >= 2
    assert not no.same_bits(a.pts[top]["iR"], b.pts[top]["iR"])


@pytest.mark.parametrize("name", list(ic.cases()))
def test_single_steps_equal_the_oracle_bit_for_bit(name):
    c, fr = ic.cases()[name], _host_run(name)
    top = c.levels - 1
    for k in sorted({0, len(fr) // 2, len(fr) - 1}):
        f = fr[k]
        o, t = _oracle_at(c, f, k), _host_at(c, f, k)
        snapped = bool(f["carry"]["snapped"]) or k == len(fr) - 1
        o.snapped = snapped
        if name != "b64":                                          # bad points at the top level, some of them neighbours
            o.pts[top]["isGood"][5:9] = 0
            o.pts[top]["isGood"][30:70:3] = 0
            t.set_state(top, o.pts[top])
        T, aff = f["result"]["T"], f["result"]["aff"]              # the pose this frame converged to: most taps are inside
        for lvl in range(top, -1, -1):
            if lvl < top:
                o.propagate_down(lvl + 1); t.propagate_down(lvl + 1, snapped)
                _same(t.points(lvl), o.pts[lvl], what=(name, k, lvl, "propagateDown"))
            o.reset_points(lvl); t.reset_points(lvl)
            _same(t.points(lvl), o.pts[lvl], what=(name, k, lvl, "resetPoints"))
            # the first loop: per tap residual and hw, the rows before the alphaOpt terms, maxstep, energy, isGood_new
            fl = o.first_loop(lvl, T[:, :3], T[:, 3], aff[0], aff[1])
            rows, taps, sums = t.first_loop(lvl, T, aff)
            P = t.points(lvl)
            assert no.same_bits(taps, fl["taps"]) or np.array_equal(np.isnan(taps), np.isnan(fl["taps"])) and \
                no.same_bits(np.nan_to_num(taps), np.nan_to_num(fl["taps"])), (name, k, lvl, "taps")
            wg = fl["was_good"]
            assert wg.sum() > 0 and no.same_bits(rows[wg], fl["row"][wg]), (name, k, lvl, "rows")
            assert no.same_bits(P["maxstep"], fl["maxstep"]) and np.array_equal(P["isGood_new"] != 0, fl["good_new"])
            assert no.same_bits(P["energy_new"][fl["good_new"], 0], fl["energy"][fl["good_new"]])
            # the whole of calcResAndGS: the rows with their alphaOpt / coupling terms and 1 / (1 + x), lastHessian_new, energy_new
            H, b, Hsc, bsc, res = o.calc(lvl, T[:, :3], T[:, 3], aff[0], aff[1])
            y = t.calc(lvl, T, aff)
            g = fl["good_new"]
            assert no.same_bits(t.jb(lvl, 1)[g], o.jb_new[lvl][g]), (name, k, lvl, "rows after the third loop")
            _same(t.points(lvl), o.pts[lvl], what=(name, k, lvl, "calcResAndGS"))
            # the sums: within n 2^-53 sum|term| of the exact sum of the same fp32 terms (the alphaOpt terms added to both)
            tm, n_terms = o.terms, 8 * max(1, o.terms["n_good"])
            e_exact = float(np.sum(tm["E"]))
            assert abs(float(sums[45]) - e_exact) <= len(tm["E"]) * 2.0 ** -53 * float(np.abs(tm["E"]).sum())
            for q, (a_, b_) in enumerate(no.TRI):
                assert abs(sums[q] - tm["acc9"][q]) <= n_terms * 2.0 ** -53 * tm["acc9_abs"][q], (name, k, lvl, q)
            assert y["res"][1] == res[1] and y["res"][2] == res[2]
            # ... and the weighted 45 of acc9SC: one term per good point; Hsc and bsc are those sums narrowed, in both triangles
            n_sc = max(1, tm["n_good"])
            for q, (a_, b_) in enumerate(no.TRI):
                assert abs(t.sc_sums[q] - tm["sc"][q]) <= n_sc * 2.0 ** -53 * tm["sc_abs"][q], (name, k, lvl, "acc9SC", q)
                want32 = np.float32(tm["sc"][q])
                for got in ((y["Hsc"][a_, b_], y["Hsc"][b_, a_]) if b_ < 8 else (y["bsc"][a_],) if a_ < 8 else ()):
                    assert abs(float(got) - float(want32)) <= float(np.spacing(np.abs(want32))), (name, k, lvl, "Hsc / bsc", a_, b_, got, want32)
                    # the reference's fp32 accumulator is within its own n eps sum|term| of the same value
                    ref = Hsc[a_, b_] if b_ < 8 else bsc[a_]
                    assert abs(float(ref) - float(want32)) <= 1.5 * n_sc * 2.0 ** -24 * tm["sc_abs"][q] + float(np.spacing(np.abs(want32)))
            assert tm["n_good"] > 0 and np.abs(tm["sc"]).max() > 0
            # the float systems: both sides round their own sum once; the oracle's fp32 accumulators carry n eps32 sum|term|
            tolH = lambda absx: 1.5 * n_terms * 2.0 ** -24 * absx + 1e-30
            for q, (a_, b_) in enumerate(no.TRI):
                got = y["H"][a_, b_] if b_ < 8 else y["b"][a_] if a_ < 8 else None
                want = H[a_, b_] if b_ < 8 else b[a_] if a_ < 8 else None
                if got is not None:
                    extra = abs(float(want)) * 2.0 ** -20 if a_ < 3 and (a_ == b_ or b_ == 8) else 0.0      # alphaOpt npts joins the entry
                    assert abs(float(got) - float(want)) <= tolH(tm["acc9_abs"][q]) + extra, (name, k, lvl, a_, b_, got, want)
            # doStep with this system's increment, calcEC, applyStep, optReg
            inc = ih.solve_inc(y, t.prm, 0.1, (c.W >> lvl) * (c.H >> lvl))
            o.jb[lvl] = t.jb(lvl, 0).copy()
            o.do_step(lvl, 0.1, inc); t.do_step(lvl, 0.1, inc)
            _same(t.points(lvl), o.pts[lvl], what=(name, k, lvl, "doStep"))
            ec_o, ec_t = o.calc_ec(lvl), t.calc_ec(lvl, snapped)
            assert ec_o[2] == ec_t[2]
            if snapped:                                            # the fp64 sum, narrowed: the exact sum's float or its neighbour
                exact = (t.prm["coupling_weight"][0] * o.ec_terms.sum(axis=0).astype(np.float32)).astype(np.float32)
                assert (np.abs(ec_t[:2] - exact) <= np.spacing(exact)).all(), (name, k, lvl, ec_t, exact)
                # ... and the reference's fp32 accumulator is within its own n eps sum|term| of it
                assert (np.abs(ec_o[:2] - exact) <= len(o.ec_terms) * 2.0 ** -24 * exact + np.spacing(exact)).all()
            o.apply_step(lvl); t.apply_step(lvl)
            _same(t.points(lvl), o.pts[lvl], what=(name, k, lvl, "applyStep"))
            assert no.same_bits(t.jb(lvl, 0)[g], o.jb[lvl][g])
            o.opt_reg(lvl); t.opt_reg(lvl, snapped)
            _same(t.points(lvl), o.pts[lvl], what=(name, k, lvl, "optReg"))
        for l in range(top):
            o.propagate_up(l); t.propagate_up(l, snapped)
            _same(t.points(l + 1), o.pts[l + 1], what=(name, k, l, "propagateUp"))
        t.close()


@pytest.mark.parametrize("name", list(ic.cases()))
def test_a_sequence_is_within_the_measured_bound_of_the_oracle(name):
    c, fr = ic.cases()[name], _host_run(name)
    o = no.Oracle(c)
    worst_T = worst_a = 0.0
    for k, f in enumerate(c.frames):
        q, r = o.track_frame(f, c.exposures[k + 1], c.exposures[0], 1), fr[k]["result"]
        dT, da = float(np.abs(r["T"] - q["T"]).max()), float(np.abs(r["aff"] - q["aff"]).max())
        worst_T, worst_a = max(worst_T, dT), max(worst_a, da)
        print(f"{name} frame {k + 1}: |dT| {dT:.3g} |daff| {da:.3g}")
        assert (int(r["snapped"]), int(r["frame_id"]), int(r["snapped_at"]), int(r["ready"])) == (q["snapped"], q["frame_id"], q["snapped_at"], q["ready"])
        assert dT <= POSE_BOUND and da <= AFF_BOUND
    print(f"{name}: worst |dT| {worst_T:.3g} |daff| {worst_a:.3g}")
