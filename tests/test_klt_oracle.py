"""Known answers of the KLT oracle (tests/np_klt_oracle.py), the numpy restatement of Tracker::trackPoints / trackPointsPyr.
CPU only: these check the oracle the GPU tests compare against."""
import numpy as np
import pytest

import np_klt_oracle as ko


def _scene(rng, H=60, W=80, n=400):
    coord = np.column_stack([rng.uniform(0, W, n), rng.uniform(0, H, n)])
    grad = rng.normal(size=(n, 2))
    return coord, grad, H, W


@pytest.mark.parametrize("r", [1, 3, 7])
def test_known_flow_from_linearised_frame(r):
    """an event frame -(Gx u + Gy v) built from the oracle's own splats gives f = (u, v): b = -M (u, v)"""
    rng = np.random.default_rng(r)
    coord, grad, H, W = _scene(rng)
    u, v = 0.37, -0.81
    gx = ko.draw_values_points(coord, grad[:, 0], H, W)
    gy = ko.draw_values_points(coord, grad[:, 1], H, W)
    frame = -(gx * u + gy * v)
    f, m = ko.track_points(coord, grad, frame, r)
    ok = ko.cond(m) <= 1e3            # the residual is b + M f: rounding in M, b times cond
    assert ok.sum() > 100
    assert np.allclose(f[ok], [u, v], rtol=0, atol=1e-12)


def test_splat_weights_clipping_edges_and_corners():
    H, W = 5, 7
    v = np.array([1.0])
    # interior: the four bilinear weights
    img = ko.draw_values_points(np.array([[2.25, 1.5]]), v, H, W, s=0)
    exp = np.zeros((H, W))
    exp[1, 2], exp[2, 2], exp[1, 3], exp[2, 3] = 0.75 * 0.5, 0.75 * 0.5, 0.25 * 0.5, 0.25 * 0.5
    assert np.array_equal(img, exp)
    # the right / bottom edge and the corner: out-of-image corners weigh 0, their clipped pixels get nothing
    for x, y, cells in (((W - 0.5), 2.0, {(2, W - 1): 0.5}), (3.0, H - 0.25, {(H - 1, 3): 0.25}),
                        (W - 0.5, H - 0.5, {(H - 1, W - 1): 0.25}), (float(W), float(H), {}), (0.0, 0.0, {(0, 0): 1.0}),
                        (float(W), 2.0, {}), (0.0, float(H), {})):
        img = ko.draw_values_points(np.array([[x, y]]), v, H, W, s=0)
        exp = np.zeros((H, W))
        for (r, c), w in cells.items():
            exp[r, c] = w
        assert np.array_equal(img, exp), (x, y)
    # contributions add in point order
    img = ko.draw_values_points(np.array([[1.0, 1.0], [1.0, 1.0], [1.0, 1.0]]), np.array([1e16, 1.0, -1e16]), H, W, s=0)
    assert img[1, 1] == (1e16 + 1.0) - 1e16


def test_splat_blur_is_gaussian_3x3_reflect101():
    img = ko.draw_values_points(np.array([[0.0, 0.0]]), np.array([1.0]), 4, 4, s=0.5)
    t = np.exp(-2.0)
    k = np.array([t, 1.0, t]) / (1 + 2 * t)
    # a unit impulse at the corner: reflect-101 mirrors the neighbour row / column onto -1
    assert img[0, 0] == pytest.approx(k[1] * k[1], rel=1e-15)
    assert img[0, 1] == pytest.approx(k[2] * k[1], rel=1e-15)
    assert img[1, 1] == pytest.approx(k[2] * k[2], rel=1e-15)


def test_patch_truncation_and_reflection():
    H, W = 9, 11
    img = np.arange(H * W, dtype=np.float64).reshape(H, W)
    p = ko.split_image_in_patches(img, np.array([[3.999, 4.0], [4.0, 3.999], [4.0, 4.0]]), 1)
    assert np.array_equal(p[0], img[3:6, 2:5])          # x 3.999 -> column 3 of the padded image = image columns 2..4
    assert np.array_equal(p[1], img[2:5, 3:6])
    assert np.array_equal(p[2], img[3:6, 3:6])
    # reflect-101 at the corner, and repeated when the window is wider than the image
    q = ko.split_image_in_patches(img, np.array([[0.0, 0.0]]), 2)[0]
    assert np.array_equal(q[2:, 2:], img[:3, :3]) and q[0, 2] == img[2, 0] and q[2, 0] == img[0, 2]
    assert list(ko.border_interpolate(np.arange(-6, 10), 4)) == [0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3]
    assert list(ko.border_interpolate(np.array([-3, 0, 4]), 1)) == [0, 0, 0]


def test_pyr_down_constant_and_hand_computed():
    c = np.full((1, 15, 15), 2.5)
    for lv in ko.pyramid_patches(c, 3):
        assert np.all(lv == 2.5)
    assert [lv.shape[-1] for lv in ko.pyramid_patches(c, 3)] == [15, 7, 3]
    assert [lv.shape[-1] for lv in ko.pyramid_patches(np.zeros((1, 53, 53)), 5)] == [53, 26, 13, 6, 3]
    # 7 -> 3 by hand: dst(y, x) = sum_ij k_i k_j src(refl(2y+i-2), refl(2x+j-2)) / 256, k = [1 4 6 4 1]
    rng = np.random.default_rng(0)
    src = rng.normal(size=(7, 7))
    k = np.array([1.0, 4.0, 6.0, 4.0, 1.0])
    refl = {-2: 2, -1: 1}
    exp = np.zeros((3, 3))
    for y in range(3):
        for x in range(3):
            for i in range(5):
                for j in range(5):
                    ry, cx = 2 * y + i - 2, 2 * x + j - 2
                    exp[y, x] += k[i] * k[j] * src[refl.get(ry, ry), refl.get(cx, cx)] / 256
    assert np.allclose(ko.pyr_down(src[None], 3)[0], exp, rtol=1e-14, atol=1e-15)


def test_pyr_radius():
    assert [ko.pyr_radius(L) for L in range(1, 6)] == [2, 4, 7, 14, 26]


def test_pyr_weights_are_one_over_scale_squared():
    """a constant patch stack keeps its level values, so each level's KLT is the same f: the sum is f (1 + 1/4 + 1/16 ...)"""
    rng = np.random.default_rng(5)
    coord, grad, H, W = _scene(rng, n=600)
    L = 3
    r = ko.pyr_radius(L)
    gx = ko.draw_values_points(coord, grad[:, 0], H, W)
    gy = ko.draw_values_points(coord, grad[:, 1], H, W)
    frame = -(gx * 0.2 + gy * 0.1)
    f, ms = ko.track_points_pyr(coord, grad, frame, L)
    # pyrDown is linear and the frame is the same linear combination of the gradient images, so every level returns (0.2, 0.1)
    ok = np.max(np.stack([ko.cond(m) for m in ms]), axis=0) <= 1e3
    assert ok.sum() > 100
    assert np.allclose(f[ok], np.array([0.2, 0.1]) * (1 + 1 / 4 + 1 / 16), rtol=0, atol=1e-12)
    assert r == 7


def test_zero_gradient_gives_nan():
    H, W = 30, 30
    coord = np.array([[5.0, 5.0], [25.0, 25.0]])
    grad = np.array([[1.0, 0.5], [0.0, 0.0]])
    f, _ = ko.track_points(coord, grad, np.ones((H, W)), 2)
    assert np.isnan(f[1]).all()


def test_cv_sum_order():
    m = np.array([[1e16, 1.0, 1.0, 1.0, -1e16, 1.0]])
    # (((1e16 + 1) + 1) + 1) then + ((-1e16) alone) then + 1
    assert ko.cv_sum(m)[0] == ((0.0 + (((1e16 + 1.0) + 1.0) + 1.0)) + -1e16) + 1.0


@pytest.mark.parametrize("shape", [(1, 6), (5, 7), (9, 70), (37, 45), (2, 2)])
def test_gaussian_blur_3x3_against_scipy_correlate1d(shape):
    """the blur every splat goes through against two separable scipy passes with the same taps and reflect-101 ("mirror") borders"""
    ndi = pytest.importorskip("scipy.ndimage")
    img = np.random.default_rng(shape[1]).normal(size=shape)
    t = np.exp(-0.5 / (0.5 * 0.5))
    k = np.array([t, 1.0, t]) / (1.0 + 2.0 * t)
    want = ndi.correlate1d(ndi.correlate1d(img, k, axis=1, mode="mirror"), k, axis=0, mode="mirror")
    got = ko.gaussian_blur_3x3(img, 0.5)
    err = np.abs(got - want).max()
    print(f"gaussian_blur_3x3 vs correlate1d {shape}: {err:.3e}")
    assert err <= 4 * np.spacing(np.abs(want).max())
