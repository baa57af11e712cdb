"""Known answers of the DepthPoints oracle (tests/np_depth_oracle.py): triangulation, the NaN skip, the filter's branches, the
statistics' quirks.  CPU only."""
import math

import numpy as np
import pytest

import depth_cases as dc
import np_depth_oracle as do


def _scene(rng, n=200):
    K = do.K_matrix(*rng.uniform([300, 300, 150, 100], [600, 600, 330, 250]))
    axis = rng.normal(size=3)
    ang = rng.uniform(0.02, 0.2)
    qv = np.append(np.sin(ang / 2) * axis / np.linalg.norm(axis), np.cos(ang / 2))
    R = do.quat_to_R(qv)
    t = rng.uniform(-0.3, 0.3, size=3)
    uv = rng.uniform([10, 10], [500, 350], size=(n, 2))
    z = rng.uniform(1.0, 4.0, size=n)
    Xk = np.linalg.inv(K) @ np.vstack([uv.T, np.ones(n)]) * z          # keyframe points
    xe = K @ (R @ Xk + t[:, None])
    return K, R, t, uv, (xe[:2] / xe[2]).T, z


@pytest.mark.parametrize("seed", range(5))
def test_exact_correspondences_triangulate_to_true_inverse_depth(seed):
    rng = np.random.default_rng(seed)
    K, R, t, uv, ef, z = _scene(rng)
    P_kf, P_ef = do.projection_matrices(K, R, t)
    for i in range(len(z)):
        x1, x2 = np.array([*uv[i], 1.0]), np.array([*ef[i], 1.0])
        inv = do.inv_depth_two_points_eucl(x1, x2, P_kf, P_ef)
        assert inv == pytest.approx(1.0 / z[i], rel=1e-12)
        assert do.inv_depth_closed_form(K, R, t, x1, x2) == pytest.approx(inv, rel=1e-12)     # the closed form = the pinv form


def test_vectorised_update_equals_literal():
    rng = np.random.default_rng(7)
    K, R, t, uv, ef, z = _scene(rng, 300)
    prm = do.Params(K, 0.5, 5.0)
    ef = ef + rng.normal(scale=0.5, size=ef.shape)
    s0 = do.init_vector(prm, 1.0 / z + rng.normal(scale=0.05, size=len(z)))
    tke = -R.T @ t
    a, b = s0.copy(), s0.copy()
    ca = do.update_literal(prm, a, uv, ef, R, t, tke)
    cb = do.update(prm, b, uv, ef, R, t, tke)
    assert ca == cb and ca["updated"] == len(z)
    np.testing.assert_allclose(b, a, rtol=1e-13, atol=0)


def test_zero_translation_is_the_nan_skip():
    rng = np.random.default_rng(3)
    K, R, _, uv, _, z = _scene(rng, 50)
    t = np.zeros(3)
    ef = uv + 1.0
    prm = do.Params(K, 1.0, 3.0)
    s = do.init_constant(prm, len(z))
    s0 = s.copy()
    c = do.update_literal(prm, s, uv, ef, R, t, t)
    assert c["skipped_nan"] == len(z) and c["updated"] == 0
    assert np.array_equal(s, s0)
    assert do.update(prm, s, uv, ef, R, t, t)["skipped_nan"] == len(z)


def test_negative_sigma2_is_restored_and_negative_mu_reset():
    # sigma2 < 0 after the update (cancellation in C1 (s2 + m^2) + C2 (sigma2 + mu^2) - mu_new^2 with tiny variances): the old sigma2
    # comes back, mu, a and b keep their new values
    st = np.array([1.842960039099899, 4.3632957857657545e-17, 2.0, 5.0])
    ran, restored, reset = do.filter_vogiatzis(1.8429600390997465, 1.827047964469223e-17, 2.0, st)
    assert ran and not reset and st[1] == 4.3632957857657545e-17 and st[2] != 2.0
    assert restored
    # mu < 0: mu = 1, sigma2 / a / b already updated
    st = np.array([-0.5, 0.01, 2.0, 5.0])
    ran, restored, reset = do.filter_vogiatzis(-0.4, 0.01, 2.0, st)
    assert ran and reset and st[0] == 1.0 and st[2] != 2.0 and st[3] != 5.0


def test_c2_zero_is_the_product_of_gaussians():
    mu, s2, z, tau2 = 0.5, 1e-4, 0.52, 2e-4
    st = np.array([mu, s2, 1e6, 1e-6])           # b / (a + b) ~ 1e-12: C2 ~ 0
    do.filter_vogiatzis(z, tau2, 2.0, st)
    s2n = 1.0 / (1.0 / s2 + 1.0 / tau2)
    assert st[0] == pytest.approx(s2n * (mu / s2 + z / tau2), rel=1e-9)
    assert st[1] == pytest.approx(s2n, rel=1e-6)


def test_statistics_quirks():
    assert do.mean_std_vector([0.7]) == (0.7, 0.0)
    x = [1.0, 2.0, 4.0, 8.0]
    m, v = do.mean_std_vector(x)
    assert m == 3.75 and v == pytest.approx(np.var(x, ddof=1), rel=1e-15)      # the variance, not the standard deviation
    x = np.arange(10.0)[::-1]
    assert do.median_idepth(x) == (5.0, 3.0)     # n/2 = 5 and n/3 = 3 (not the third quartile)
    assert do.median_idepth([2.0]) == (2.0, 2.0)


def test_init_overloads():
    prm = do.Params(do.K_matrix(400, 400, 160, 120), 1.0, 3.0, 100.0)
    s = do.init_constant(prm, 3)
    assert np.array_equal(s[0], [1.0, 4.0, 2.0, 5.0])
    s = do.init_vector(prm, [0.4, 0.6])
    assert np.array_equal(s[:, 0], [0.4, 0.6]) and s[0, 1] == 4.0 / 36.0
    assert prm.px_error_angle == 2 * math.atan(3.0 / 800.0)
    assert do.is_converged([0.5, 3.9e-4, 2, 5], prm.mu_range, 100.0) and not do.is_converged([0.5, 4e-4, 2, 5], prm.mu_range, 100.0)


# ---- the rare-branch scenes of tests/depth_cases.py: what the device tests rely on, established on the oracle alone ---------------
_CLS = {}


def _classified(name):
    if name not in _CLS:
        case = dc.make_case(name)
        _CLS[name] = (case, [dc.classify(s) for s in case])
    return _CLS[name]


def _totals(name):
    case, cls = _classified(name)
    t = dict(N=0, special=0, skipped=0, skipped_special=0, updated_special=0, restored=0, reset=0, reset_special=0, converged=0,
             not_converged=0, c1_zero=0, clamped=0, unclamped=0, und=0, nonfinite=0)
    for s, (ev, evx, und) in zip(case, cls):
        run = ev["run"]
        t["N"] += s.N; t["special"] += int(s.special.sum())
        t["skipped"] += int((~run).sum()); t["skipped_special"] += int((~run & s.special).sum()); t["updated_special"] += int((run & s.special).sum())
        t["restored"] += int(ev["restored"].sum()); t["reset"] += int(ev["reset"].sum()); t["reset_special"] += int((ev["reset"] & s.special).sum())
        t["converged"] += int(ev["converged"].sum()); t["not_converged"] += int((~ev["converged"]).sum())
        t["c1_zero"] += int((run & (ev["C1"] == 0.0)).sum())
        t["und"] += int((und["restore"] | und["reset"] | und["converged"]).sum())
        t["nonfinite"] += int((~np.isfinite(ev["seeds"])).any(axis=1).sum())
    return t


@pytest.mark.parametrize("name", dc.CASES)
def test_case_takes_its_branches(name):
    """the floors: each case must reach the branch it was built for, in the oracle, or the device test above it pins nothing"""
    t = _totals(name)
    if name == "zero_translation":
        assert t["skipped"] == t["N"]                                   # t = 0: alpha = acos(0 / 0) for every point, by construction
    elif name == "epipole":
        assert t["skipped"] == t["skipped_special"] == t["special"] > 0 and t["skipped"] < t["N"] // 10     # exactly the points at K t
    elif name == "zero_disparity":
        # +-0 skips (depth = inf, beta = acos(inf / inf)), dust updates: both happen, which the rounding of K K^-1 x decides per point
        assert t["skipped"] == t["skipped_special"] and t["skipped_special"] >= t["special"] // 10 and t["updated_special"] >= t["special"] // 10
    elif name == "negative_mu_seed":
        assert t["reset_special"] >= t["special"] // 2 and t["reset"] == t["reset_special"]     # mu_new = C1 m + C2 mu with mu < 0: most
    elif name == "negative_z":
        assert t["reset"] >= 10                                         # ~1 % of the moved points: only where tau2 is small enough for m ~ z
    elif name == "outliers":
        assert t["c1_zero"] >= 5 and t["reset"] >= 5                   # exp underflows to 0 on a few (11); a handful (7) resets
    elif name == "converged_seeds":
        assert t["converged"] == t["N"] and t["restored"] == 0
    elif name == "cancellation":
        assert t["restored"] >= t["N"] // 5 and t["restored"] <= 4 * t["N"] // 5      # about a third: rounding noise decides
    elif name == "threshold_edge":
        assert t["converged"] >= t["N"] // 5 and t["not_converged"] >= t["N"] // 5    # both sides of (mu_range / threshold)^2
    elif name == "tau_clamp":
        case, cls = _classified(name)
        lo = hi = 0
        for s, (ev, _, _) in zip(case, cls):
            with np.errstate(all="ignore"):
                depth = 1.0 / ev["inv_depth"]
                # tau2 = (0.5 (1 / max(1e-12, depth - tau) - 1 / (depth + tau)))^2 >= (0.25e12)^2 only through the clamp
                lo += int((ev["tau2"] > 1e22).sum()); hi += int(((ev["tau2"] < 1e22) & (depth > 0)).sum())
        assert lo >= t["N"] // 20 and hi >= t["N"] // 4                # the constant on the tiny baselines, the difference on the large
    elif name == "ab_range":
        case, _ = _classified(name)
        ab = np.concatenate([s.seeds[:, 2:] for s in case])
        assert ab.min() >= 0.1 and ab.max() <= 1e3 and (ab > 300).sum() >= 100 and (ab < 0.3).sum() >= 100
    assert t["skipped"] + sum(int(c[0]["run"].sum()) for c in _classified(name)[1]) == t["N"]


@pytest.mark.parametrize("name", dc.CASES)
def test_case_is_finite_and_decided(name):
    """every case but `cancellation` leaves finite seeds and at most 1 % of undecided branches: the device test compares nearly every
    point strictly"""
    t = _totals(name)
    if name == "cancellation":
        assert t["und"] >= t["N"] // 2          # sigma2 = 1e-17 mu^2 and below: under the rounding of the cancellation, by construction
        return
    assert t["nonfinite"] == 0
    assert t["und"] <= t["N"] // 100, t


@pytest.mark.parametrize("name", dc.CASES)
def test_vectorised_update_equals_literal_on_case(name):
    """`update` against the one-point-at-a-time `update_literal` (cv::Mat form, pinv for the inverse), three small slots per case:
    the same skip set, flags and counts, the seeds within the comparator's tolerances (pinv's K^-1 is the closed form's to an ulp).
    Where x_ef == x_kf (`zero_disparity`) that ulp triangulates OTHER dust, so there the literal form takes the closed-form K^-1 and
    row-wise products: then its skip set must be `update`'s exactly, dust points included."""
    for b, s in enumerate(dc.make_case(name, n_slots=3, n0=90)):
        cls = dc.classify(s)
        lit = s.seeds.copy()
        cnt = do.update_literal(s.oracle_params(), lit, s.kf_xy, s.ef_xy, *s.geometry(), closed_form_inverse=name == "zero_disparity")
        flags = dc.compare(s, lit, cls, restore_by_invariants=name == "cancellation")
        assert cnt["skipped_nan"] == int(flags["skipped"].sum()) and cnt["updated"] == s.N - cnt["skipped_nan"]
        assert cnt["sigma2_restored"] == int(flags["restored"].sum()) and cnt["mu_reset"] == int(flags["reset"].sum())
        vec = s.seeds.copy()
        want = do.update(s.oracle_params(), vec, s.kf_xy, s.ef_xy, *s.geometry())
        if name == "cancellation":          # the restore decision is rounding noise: every other count must agree
            cnt.pop("sigma2_restored"); want.pop("sigma2_restored")
        assert cnt == want
        if name == "zero_disparity":
            assert 0 < cnt["skipped_nan"] < int(s.special.sum())


def test_sigma2_allowance_measurement():
    """the constants of depth_cases.py, re-measured: max |fp64 - extended| of the pre-branch sigma2_new in units of
    2^-52 (mu_new^2 + m^2), and of a_new in units of 2^-52 f / |f - e / f| relative, over the points REL does not already cover"""
    s2_units = ab_units = raw_units = raw_rel = 0.0
    where = {}
    for name in dc.CASES:
        case, cls = _classified(name)
        for s, (ev, evx, _) in zip(case, cls):
            well = dc.well_conditioned(ev, evx)
            with np.errstate(all="ignore"):
                d = np.abs(ev["sigma2_new"] - evx["sigma2_new"]).astype(np.float64)
                if well.any():
                    raw_units = max(raw_units, float((d / (dc.EPS * dc.sigma2_scale(ev)))[well].max()))
                    if name not in ("converged_seeds", "cancellation"):
                        raw_rel = max(raw_rel, float((d / np.abs(ev["sigma2_new"]))[well].max()))
                need = well & (d > dc.REL * np.abs(ev["sigma2_new"]))
                if need.any():
                    u = float((d / (dc.EPS * dc.sigma2_scale(ev)))[need].max())
                    where[name] = max(where.get(name, 0.0), u)
                    s2_units = max(s2_units, u)
                for key in ("a_new", "b_new"):
                    r = (np.abs(ev[key] - evx[key]) / np.abs(evx[key])).astype(np.float64)
                    need = well & (r > dc.REL)
                    if need.any():
                        assert name == "ab_range"
                        ab_units = max(ab_units, float((r / (dc.EPS * np.abs(ev["f"] / (ev["f"] - ev["e"] / ev["f"]))))[need].max()))
                r = (np.abs(ev["mu_new"] - evx["mu_new"]) / np.abs(evx["mu_new"])).astype(np.float64)
                assert not (well & (r > dc.REL)).any()              # mu needs no allowance
    print("sigma2 units", s2_units, where, "a/b units", ab_units, "raw units", raw_units, "raw relative outside the cancelling cases", raw_rel)
    # the raw maximum, REL-covered points included, is conditioning (relative to sigma2, far inside REL), not cancellation
    assert raw_units > 1000.0 * dc.SIGMA2_UNITS_MEASURED and raw_rel < 0.1 * dc.REL
    assert set(where) <= {"converged_seeds", "cancellation"}
    assert 0.9 * dc.SIGMA2_UNITS_MEASURED <= s2_units <= dc.SIGMA2_UNITS_MEASURED
    assert 0.9 * dc.AB_UNITS_MEASURED <= ab_units <= dc.AB_UNITS_MEASURED
    assert dc.SIGMA2_ALLOWANCE_UNITS == 4.0 * dc.SIGMA2_UNITS_MEASURED and dc.AB_ALLOWANCE_UNITS == 4.0 * dc.AB_UNITS_MEASURED


def test_free_run_allowance_measurement():
    """60 free-running steps in fp64 and in extended precision on the same tracks: mu, a and b stay within REL, sigma2 does NOT (the
    narrowed seeds reach sigma2 / mu^2 ~ 1e-7, where the cancellation's accumulated error shows); its excess, in units of
    2^-52 2 mu^2 over all steps, is the constant the device test's allowance is 4 x of"""
    als, idp0, poses = dc.free_run_scene()
    h64, planes = dc.free_run_oracle(als, idp0, poses)
    hx, _ = dc.free_run_oracle(als, idp0, poses, np.longdouble, planes)
    units = worst_rel = 0.0
    first = None
    for step in range(dc.FREE_RUN_STEPS):
        for s, x in zip(h64[step], hx[step]):
            assert np.isfinite(s).all()
            rel = (np.abs(s - x) / np.abs(x)).astype(np.float64)
            assert rel[:, [0, 2, 3]].max() <= dc.REL
            worst_rel = max(worst_rel, float(rel[:, 1].max()))
            need = rel[:, 1] > dc.REL
            if need.any():
                first = step + 1 if first is None else first
                units = max(units, float((np.abs(s[:, 1] - x[:, 1]).astype(np.float64) / (dc.EPS * 2.0 * s[:, 0] ** 2))[need].max()))
    print("sigma2 leaves REL at step", first, "max relative difference", worst_rel, "units", units)
    assert first is not None and worst_rel > dc.REL                     # REL cannot hold for sigma2 here: the oracle itself misses it
    assert 0.9 * dc.FREE_RUN_UNITS_MEASURED <= units <= dc.FREE_RUN_UNITS_MEASURED
    assert dc.FREE_RUN_ALLOWANCE_UNITS == 4.0 * dc.FREE_RUN_UNITS_MEASURED
