"""Known answers of the DepthPoints oracle (tests/np_depth_oracle.py): triangulation, the NaN skip, the filter's branches, the
statistics' quirks.  CPU only."""
import math

import numpy as np
import pytest

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
