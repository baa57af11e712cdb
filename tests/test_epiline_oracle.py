"""Hand-computed cases for the numpy restatement of trackPointsAlongEpiline (tests/np_epiline_oracle.py): the normed scores, each
branch of the clamp rule, zero windows and templates, the tie rules, the borders and the truncation that places a template.
No GPU needed."""
import numpy as np
import pytest

import np_epiline_oracle as eo
import subpixel_cases as sc


def _maps(img, tmpl, r, border=eo.BORDER_CONSTANT, value=0):
    padded = eo.copy_make_border(np.asarray(img, np.float64), r, border, value).astype(np.float32)
    return eo.score_maps(padded, np.asarray(tmpl, np.float32)[None])


def test_both_normed_scores_r0():
    # r = 0: C = p t, E = p^2, S = t^2, so |C| == t: CCORR lands on the +-1 branch; SQDIFF = (p - t)^2 / |p t|
    img = np.array([[1.0, 2.0], [3.0, 4.0]])
    ssd, ncc = _maps(img, [[2.0]], 0)
    assert np.array_equal(ncc[0], np.ones((2, 2), np.float32))
    want = np.float32([[1.0 / 2.0, 0.0], [1.0 / 6.0, 4.0 / 8.0]])
    assert np.array_equal(ssd[0], want)
    out = eo.match(img, np.float32([[[2.0]]]), 0, eo.BORDER_CONSTANT, 0)
    assert tuple(out["ssd"][0]) == (1, 0) and out["s_ssd"][0] == 0.0
    assert tuple(out["ncc"][0]) == (0, 0)                    # every position ties at 1: the first wins


def test_scores_on_a_small_image():
    # 3 x 3 image, r = 1, template = the image's centre window: exact match at the centre
    img = np.arange(1.0, 10.0).reshape(3, 3)
    T = img.astype(np.float32)
    ssd, ncc = _maps(img, T, 1)
    P = eo.copy_make_border(img, 1, eo.BORDER_CONSTANT, 0)
    y, x = 0, 2
    win = P[y:y + 3, x:x + 3]
    C, E, S = float((win * T).sum()), float((win * win).sum()), float((T * T).sum())
    t = np.sqrt(E) * np.sqrt(S)
    assert ncc[0, y, x] == np.float32(C / t)
    num = (E - 2 * C) + S
    assert ssd[0, y, x] == np.float32(num / t if num < t else 1.0)
    assert ssd[0, 0, 1] == np.float32(((E1 := float((P[0:3, 1:4] ** 2).sum())) - 2 * float((P[0:3, 1:4] * T).sum()) + S)
                                      / (np.sqrt(E1) * np.sqrt(S)))
    assert ssd[0, 1, 1] == 0.0                               # the exact match
    out = eo.match(img, T[None], 1, eo.BORDER_CONSTANT, 0)
    assert tuple(out["ssd"][0]) == (1, 1)


@pytest.mark.parametrize("C,E,S,want_ncc,ssd_branch", [
    (1.0, 4.0, 1.0, 0.5, "one"),            # |C| < t = 2: C / t; num = 3 >= t: ssd 1
    (2.1, 4.0, 1.0, 1.0, "ratio"),          # t <= C < 1.125 t: +1; num = 0.8 < t: num / t
    (-2.1, 4.0, 1.0, -1.0, "one"),          # -1; num = 9.2 >= t
    (2.3, 4.0, 1.0, 0.0, "ratio"),          # C >= 1.125 t: 0
    (1.9, 4.0, 1.0, 0.95, "ratio"),
    (3.0, 4.0, 1.0, 0.0, "zero"),           # num < 0 -> max(num, 0) = 0
])
def test_clamp_branches(C, E, S, want_ncc, ssd_branch):
    ssd, ncc = eo.normed_scores(C, E, S)
    t = np.sqrt(E) * np.sqrt(S)
    assert ncc == np.float32(C / t if abs(C) < t else want_ncc)
    want = {"one": 1.0, "zero": 0.0, "ratio": ((E - 2.0 * C) + S) / t}[ssd_branch]
    assert ssd == np.float32(want)


def test_zero_window_and_zero_template():
    # t = 0: CCORR 0, SQDIFF 1 (num < 0 is false, num < 1.125 t is false)
    ssd, ncc = eo.normed_scores(0.0, 0.0, 5.0)
    assert ncc == 0.0 and ssd == 1.0
    ssd, ncc = eo.normed_scores(0.0, 5.0, 0.0)
    assert ncc == 0.0 and ssd == 1.0
    # a NaN window scores like a zero one: every comparison is false
    ssd, ncc = eo.normed_scores(np.nan, np.nan, 1.0)
    assert ncc == 0.0 and ssd == 1.0


def test_zero_template_ties_at_one_and_goes_to_origin():
    rng = np.random.default_rng(0)
    img = rng.normal(size=(6, 7))
    out = eo.match(img, np.zeros((1, 3, 3), np.float32), 1, eo.BORDER_REFLECT_101, 0)
    assert tuple(out["ssd"][0]) == (0, 0) and out["s_ssd"][0] == 1.0
    assert tuple(out["ncc"][0]) == (0, 0) and out["s_ncc"][0] == 0.0
    assert out["keep"][0]


def test_zero_velocity_keeps_every_point_at_origin():
    rng = np.random.default_rng(1)
    H, W, n = 20, 24, 12
    kp = np.column_stack([rng.integers(0, W, n), rng.integers(0, H, n)]).astype(np.float64)
    out = eo.track_points_along_epiline(kp, rng.normal(size=(n, 2)), rng.uniform(0.5, 1, n), np.zeros(6), (20.0, 20.0, 12.0, 10.0),
                                        rng.normal(size=(H, W)), r=2)
    assert np.array_equal(out["ssd"], np.zeros((n, 2))) and np.array_equal(out["ncc"], np.zeros((n, 2)))
    assert out["keep"].all()


def test_row_major_tie_order():
    # two exact matches: (x=4, y=1) and (x=1, y=3); row-major order puts y = 1 first although its x is larger
    img = np.zeros((5, 6))
    img[1, 4] = 3.0
    img[3, 1] = 3.0
    m = np.zeros((5, 6), np.float32)
    m[1, 4] = 0.5
    m[3, 1] = 0.5
    assert eo.arg_best(m, False)[0] == (0, 0)
    assert eo.arg_best(m, True)[0] == (4, 1)
    out = eo.match(img, np.float32([[[3.0]]]), 0, eo.BORDER_CONSTANT, 0)
    assert tuple(out["ssd"][0]) == (4, 1) and tuple(out["ncc"][0]) == (4, 1)
    # -0 and +0 tie: the first wins
    z = np.float32([[0.0, -0.0], [-0.0, 0.0]])
    assert eo.arg_best(z, True)[0] == (0, 0) and eo.arg_best(z, False)[0] == (0, 0)


def test_no_finite_score_reports_minus_one_and_fails_the_cull():
    (xy, s) = eo.arg_best(np.full((2, 2), np.nan, np.float32), False)
    assert xy == (-1, -1) and np.isnan(s)
    assert not eo.cull([[-1, -1]], [[-1, -1]])[0]
    assert eo.cull([[3, 4]], [[0, 5]])[0]                      # equal norms
    assert not eo.cull([[0, 0]], [[6, 0]])[0]                  # 6 > 5
    assert eo.cull([[0, 0]], [[5, 0]])[0]                      # exactly 5 is kept


def test_each_border_type():
    row = np.array([[1.0, 2.0, 3.0, 4.0]])
    want = {
        eo.BORDER_CONSTANT: [9, 9, 1, 2, 3, 4, 9, 9],
        eo.BORDER_REPLICATE: [1, 1, 1, 2, 3, 4, 4, 4],
        eo.BORDER_REFLECT: [2, 1, 1, 2, 3, 4, 4, 3],
        eo.BORDER_REFLECT_101: [3, 2, 1, 2, 3, 4, 3, 2],
    }
    for border, w in want.items():
        p = eo.copy_make_border(row, 2, border, 9)
        assert np.array_equal(p[2], np.array(w, np.float64)), border
    # a window wider than the image keeps reflecting
    assert list(eo.border_index(np.arange(-5, 8), 3, eo.BORDER_REFLECT_101)) == [1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1]
    assert list(eo.border_index(np.arange(-4, 7), 3, eo.BORDER_REFLECT)) == [2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0]


def test_truncation_places_templates_at_the_integer_pixel():
    # fx ((u - cx) / fx) + cx can land 1e-13 below an integer u: the slot's cell + fp32 fraction gives u back exactly
    fx, cx = 458.6548807207614, 367.2158039615726
    found = 0
    for u in range(0, 640):
        nx = (u - cx) / fx
        back = fx * nx + cx
        if back < u:
            found += 1
            px = eo.slot_pixels(np.array([[nx, nx]]), fx, fx, cx, cx)
            assert px[0, 0] == float(u) and int(np.trunc(px[0, 0])) == u
    assert found > 0
    model = np.arange(30.0).reshape(5, 6)
    t = eo.templates(model, np.array([[2.9999999, 1.0], [3.0, 1.0]]), 1, eo.BORDER_REFLECT_101, 0)
    assert np.array_equal(t[0], model[0:3, 1:4].astype(np.float32)) and np.array_equal(t[1], model[0:3, 2:5].astype(np.float32))


def test_sparse_model_normalisation_and_order():
    kp = np.array([[3.0, 4.0], [10.0, 2.0], [7.0, 7.0]])
    g = np.array([[1.0, 0.0], [0.0, 2.0], [1.0, 1.0]])
    v = np.array([0.1, -0.2, 0.3, 0.01, 0.02, -0.03])
    K = (10.0, 10.0, 5.0, 5.0)
    m = eo.sparse_model(kp, g, np.ones(3), v, K)
    x, y = (kp[:, 0] - 5.0) / 10.0, (kp[:, 1] - 5.0) / 10.0
    f0 = -v[0] + x * v[2] + x * y * v[3] - (1 + x * x) * v[4] + y * v[5]
    f1 = -v[1] + y * v[2] + (1 + y * y) * v[3] - x * y * v[4] - x * v[5]
    raw = -(g[:, 0] * f0 + g[:, 1] * f1)
    assert np.allclose(m, raw / np.sqrt(1e-3 + (raw * raw).sum()), rtol=1e-14, atol=0)
    assert np.array_equal(eo.sparse_model(kp, g, np.ones(3), np.zeros(6), K), np.zeros(3))


# -- the inputs of the sub-pixel GPU tests (tests/subpixel_cases.py), checked before they reach a GPU ----------------------------------

def test_subpixel_helper_promises():
    for H, W in sc.FRAMES + [(480, 640)]:
        al = sc.subpixel_alignment(3, H, W, 400)
        kp = eo.slot_pixels(al.norm_coord, al.fx, al.fy, al.cx, al.cy)
        assert np.abs(kp - al.coord).max() < 1e-4
        assert (kp[:, 0] >= 1).all() and (kp[:, 0] <= W - 2).all() and (kp[:, 1] >= 1).all() and (kp[:, 1] <= H - 2).all()
        fr = kp - np.floor(kp)
        off_grid = ((fr >= 0.05) & (fr <= 0.95)).all(axis=1)
        assert off_grid.mean() >= 0.7, (H, W, off_grid.mean())
        for name in ("SEAMS", "LAST", "JUST_OUTSIDE"):
            pts = np.array(getattr(sc, name)(H, W))
            assert len(pts) > 0, (name, H, W)
        s = np.array(sc.SEAMS(H, W))
        assert set(np.floor(s[:, 0])) >= {v for v in (31, 32, 63, 64) if v < W} and (s[:, 0] < W).all() and (s[:, 1] < H).all()
        assert set(np.floor(s[:, 1])) >= {v for v in (7, 8, 15, 16, 31, 32) if v < H}
        assert set((s - np.floor(s)).ravel()) <= {0.25, 0.5, 0.75}
        la = np.array(sc.LAST(H, W))
        assert {(W - 1.0, H - 1.0), (W - 0.5, H - 0.5), (W - 1.0, H - 0.5), (W - 0.5, H - 1.0)} <= set(map(tuple, la))
        jo = np.array(sc.JUST_OUTSIDE(H, W))
        assert ((jo[:, 0] > -1) & (jo[:, 0] < 0) & (jo[:, 1] > 0) & (jo[:, 1] < H - 1)).any()
        assert ((jo[:, 1] > -1) & (jo[:, 1] < 0) & (jo[:, 0] > 0) & (jo[:, 0] < W - 1)).any()
        assert ((jo[:, 0] < 0) & (jo[:, 1] < 0)).any() and (jo[:, 0] > W).any() and (jo[:, 1] > H).any()
        # `extra` is appended verbatim, and EXACT holds a pixel the slot stores as cell k - 1 with the fp32 fraction 1.0f
        al = sc.subpixel_alignment(4, H, W, 10, extra=sc.EXACT)
        assert al.N == 10 + len(sc.EXACT) and np.array_equal(al.coord[10:], np.array(sc.EXACT))
        ex = np.array(sc.EXACT)
        assert (ex[:, 0] < W - 1).all() and (ex[:, 1] < H - 1).all()
        u = np.column_stack([al.fx * al.norm_coord[10:, 0] + al.cx, al.fy * al.norm_coord[10:, 1] + al.cy])
        kp = eo.slot_pixels(al.norm_coord[10:], al.fx, al.fy, al.cx, al.cy)
        below = (u < np.rint(u)) & (kp == np.rint(u))
        assert below.any(), (H, W)
        assert (kp == np.rint(kp)).all(axis=1).sum() >= 3
    assert sc.subpixel_alignment(5, 37, 45, 0, extra=sc.JUST_OUTSIDE(37, 45)).N == len(sc.JUST_OUTSIDE(37, 45))


def _parity_case_oracle(H, W, r, border, value):
    """the oracle alone on the construction of test_parity_subpixel_odd_frames (tests/test_epiline_gpu.py): its own model image,
    shifted by (2, -1), 5 % noise with seed r, as the fp32 frame a slot holds"""
    al = sc.parity_alignment(H, W)
    frame = sc.f32(sc.shifted_frame(sc.oracle_model(al), seed=r))
    kp = eo.slot_pixels(al.norm_coord, al.fx, al.fy, al.cx, al.cy)
    return eo.track_points_along_epiline(kp, sc.f32(al.grad), sc.f32(al.idp), sc.VEL, (al.fx, al.fy, al.cx, al.cy), frame, r, border,
                                         value, with_maps=True)


def test_parity_case_table_is_the_issue_s():
    cases = set(sc.PARITY_CASES)
    assert len(cases) == len(sc.PARITY_CASES) == 3 * 4 * 3 + (3 + 4) * 2
    for H, W in sc.ODD_FRAMES:
        for r in (0, 3, 7, 15):
            for b in (eo.BORDER_REPLICATE, eo.BORDER_REFLECT, eo.BORDER_REFLECT_101):
                assert (H, W, r, b, 0) in cases
            for v in (0, 255):
                assert ((H, W, r, eo.BORDER_CONSTANT, v) in cases) == ((H, W) == (37, 45) or ((H, W) == (61, 83) and r <= 7))


@pytest.mark.parametrize("H,W,r,border,value", sc.PARITY_CASES)
def test_parity_case_table_strict_shares(H, W, r, border, value):
    """every committed case leaves at least half of its points with a strict best match, so the device is judged on the location of
    those (at r = 0 every CCORR score is +-1: nothing is strict, only the tie rule applies)"""
    ref = _parity_case_oracle(H, W, r, border, value)
    assert len(ref["ssd"]) == sc.PARITY_N
    s_ssd = sc.strict_share(ref["ssd_map"], ref["ssd"], r, False)
    s_ncc = sc.strict_share(ref["ncc_map"], ref["ncc"], r, True)
    print(f"strict shares {H}x{W} r={r} border={border}/{value}: ssd {s_ssd:.3f} ncc {s_ncc:.3f}")
    assert s_ssd >= 0.5
    if r >= 1:
        assert s_ncc >= 0.5


# -- the oracle against independent restatements of its padding and its correlation ---------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 6), (5, 7), (9, 70), (37, 45)])
@pytest.mark.parametrize("r", [0, 1, 3, 7, 15])
def test_copy_make_border_equals_np_pad(shape, r):
    img = np.random.default_rng(shape[0] + r).normal(size=shape)
    for border, mode, kw in ((eo.BORDER_REPLICATE, "edge", {}), (eo.BORDER_REFLECT, "symmetric", {}), (eo.BORDER_REFLECT_101, "reflect", {}),
                             (eo.BORDER_CONSTANT, "constant", dict(constant_values=255.0)), (eo.BORDER_CONSTANT, "constant", dict(constant_values=0.0))):
        got = eo.copy_make_border(img, r, border, kw.get("constant_values", 0))
        assert got.shape == (shape[0] + 2 * r, shape[1] + 2 * r)
        assert np.array_equal(got, np.pad(img, r, mode=mode, **kw)), (border, kw)


@pytest.mark.parametrize("r", [0, 1, 3, 7])
def test_score_maps_against_scipy_correlate2d(r):
    sig = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(20 + r)
    P = rng.normal(size=(19 + 2 * r, 23 + 2 * r)).astype(np.float32)
    T = rng.normal(size=(3, 2 * r + 1, 2 * r + 1)).astype(np.float32)
    ssd, ncc = eo.score_maps(P, T)
    P64 = P.astype(np.float64)
    E = sig.correlate2d(P64 * P64, np.ones((2 * r + 1, 2 * r + 1)), mode="valid")
    worst = 0.0
    for i in range(3):
        T64 = T[i].astype(np.float64)
        C = sig.correlate2d(P64, T64, mode="valid")
        S = float((T64 * T64).sum())
        t = np.sqrt(E) * np.sqrt(S)
        num = np.maximum(E - 2.0 * C + S, 0.0)
        if r >= 1:
            # no clamp branch is near its threshold: |C| < t and num >= t (or num < t) with room to spare
            assert (np.abs(C) < t * (1 - 1e-6)).all() and (np.abs(num - t) > 1e-6 * t).all()
            want_ncc = C / t
        else:
            # one pixel: |C| = |P||T| = t up to rounding, the +-1 branch (|C| < 1.125 t) with room to spare
            assert (np.abs(np.abs(C) - t) <= 1e-12 * t).all() and (np.abs(num - t) > 1e-6 * t).all()
            want_ncc = np.sign(C)
        want_ssd = np.where(num < t, num / t, 1.0)
        assert (np.abs(want_ncc) <= 1).all() and (want_ssd >= 0).all() and (want_ssd <= 1).all()
        worst = max(worst, np.abs(ncc[i].astype(np.float64) - want_ncc).max(), np.abs(ssd[i].astype(np.float64) - want_ssd).max())
    print(f"score_maps vs correlate2d, r={r}: {worst:.3e}")
    assert worst <= 2.0 ** -24 + 1e-12
