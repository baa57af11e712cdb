"""The numpy restatement of include/eds_hip_kfpoints.h (tests/np_kfpoints_oracle.py) on its own, and — on the oracle alone — that the
cases the GPU test runs (tests/kfpoints_cases.py) discriminate: a refine case erases and keeps a tenth of its points at least and has
points whose fate hangs on the radius, the border rule and the truncation; no clean weight is undecided; the projection throws points
out through every side and behind the camera, and none lands within 1e-6 px of the destination frame's edge."""
import numpy as np
import pytest

import kfpoints_cases as kc
import np_kfpoints_oracle as kp
import subpixel_cases as sc


def _brute_range(frame, tx, ty, r, border, value):
    """tap by tap, python loops: an independent restatement of window_range"""
    H, W = frame.shape
    out = []
    for x, y in zip(tx, ty):
        lo = hi = None
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                yy, xx = y + dy, x + dx
                if border == kp.BORDER_CONSTANT and not (0 <= yy < H and 0 <= xx < W):
                    v = np.float32(value)
                else:
                    v = np.float32(frame[int(kp.border_index([yy], H, border)[0]), int(kp.border_index([xx], W, border)[0])])
                if np.isnan(v):
                    continue
                lo = v if lo is None or v < lo else lo
                hi = v if hi is None or v > hi else hi
        out.append(np.nan if lo is None else abs(float(hi) - float(lo)))
    return np.array(out)


@pytest.mark.parametrize("border,value", kc.BORDERS)
def test_window_range_against_loops(border, value):
    rng = np.random.default_rng(3)
    f = kc.stored(rng.standard_normal((9, 14)))
    f[2:5, 3:9] = np.nan                                        # a NaN patch: r = 1 windows inside it have no finite tap
    tx = np.array([0, 13, 5, 5, -1, 14, 7, -40, 3])
    ty = np.array([0, 8, 3, 4, 4, -1, 20, 2, 3])
    for r in (0, 1, 3, 6):
        a = kp.window_range(f, (tx, ty), r, border, value)
        b = _brute_range(f, tx, ty, r, border, value)
        assert np.array_equal(a, b, equal_nan=True), (r, a, b)
    rng1, keep = kp.refine(f, np.column_stack([tx, ty]).astype(np.float64), 0.5, 1, border, value)
    assert np.isnan(rng1[2]) and keep[2]                        # (5, 3): all nine taps NaN -> NaN range -> kept
    assert np.array_equal(keep, ~(rng1 < 0.5))


def test_truncation_is_towards_zero_on_the_slot_pixel():
    al, idx = kc.refine_points(61, 83)
    kpix = kp.slot_pixels(al.norm_coord, al.fx, al.fy, al.cx, al.cy)
    tx, ty = kp.truncated(kpix)
    fx, fy = kc.floor_centres(al)
    neg = [i for i in idx["outside"] if -1 < al.coord[i, 0] < 0]
    assert len(neg) and all(tx[i] == 0 and fx[i] == -1 for i in neg)
    below = [i for i in idx["exact"] if al.coord[i, 0] != np.round(al.coord[i, 0])]
    assert len(below) and all(tx[i] == np.round(al.coord[i, 0]) and fx[i] == tx[i] - 1 for i in below)
    assert kp.truncated(np.array([[3e9, -3e9]])) == (np.array([2 ** 20]), np.array([-2 ** 20]))


@pytest.mark.parametrize("H,W", kc.FRAMES)
@pytest.mark.parametrize("r", [r for r in kc.RADII if r >= 1])
def test_refine_cases_discriminate(H, W, r):
    c = kc.refine_conditions(H, W, r, kc.REFINE_SEEDS.get((H, W, r), 0))
    print(H, W, r, c)
    assert 0.1 <= c["erased"] <= 0.9, c
    assert c["flips_radius"] >= 1 and c["flips_border"] >= 1, c
    assert c["flips_floor_negative"] >= 1 and c["flips_floor_exact"] >= 1, c


@pytest.mark.parametrize("H,W", kc.FRAMES)
def test_refine_radius_zero_erases_everything(H, W):
    al, _ = kc.refine_case(H, W, 0)
    kpix = kp.slot_pixels(al.norm_coord, al.fx, al.fy, al.cx, al.cy)
    for border, value in kc.BORDERS:
        rng, keep = kp.refine(kc.stored(al.frame), kpix, kc.EVENT_DIFF, 0, border, value)
        assert np.all(rng == 0.0) and not keep.any()


def test_refine_case_ranges_are_far_from_the_threshold():
    """a range is 0, a spike's amplitude (>= AMP_MIN) or more: event_diff sits a quarter of a unit from both"""
    for H, W in kc.FRAMES:
        for r in kc.RADII:
            al, _ = kc.refine_case(H, W, r)
            kpix = kp.slot_pixels(al.norm_coord, al.fx, al.fy, al.cx, al.cy)
            for border, value in kc.BORDERS:
                rng = kp.refine(kc.stored(al.frame), kpix, kc.EVENT_DIFF, r, border, value)[0]
                assert np.all((rng == 0.0) | (rng >= kc.AMP_MIN - 1e-6)), (H, W, r, border)


def test_clean_cases_have_no_undecided_weight():
    for seed in (0, 1, 2):
        w = kc.clean_weights(seed, 700)
        w32 = w.astype(np.float32).astype(np.float64)
        for t in kc.CLEAN_THRESHOLDS:
            assert np.abs(w32 - t).min() > 1e-6 and np.abs(w - t).min() > 1e-6
            keep = kp.clean(w, t)
            assert np.array_equal(keep, ~(w < t))               # the fp32 rule and the reference's fp64 comparison agree
            assert 0.1 <= keep.mean() <= 0.9


def test_erase_takes_a_mask_or_indices():
    m = np.zeros(10, bool)
    m[[2, 7, 9]] = True
    assert np.array_equal(kp.erase(10, m), kp.erase(10, [9, 2, 7])) and kp.erase(10, m).sum() == 7
    assert kp.erase(4, []).all()


def test_num_points_rules():
    s = kp.NumPoints()
    s.build_keyframe(1000, 640)
    assert (s.num_points, s.current) == (1000, 640)
    assert s.need_new_kf(0.1) and not s.need_new_kf(0.36) and s.need_new_kf(0.3599)       # 360 > thr * 1000
    s.refine(500)
    assert (s.num_points, s.current) == (500, 500) and not s.need_new_kf(0.1)
    s.refine(500, erased=False)
    s.erased(451)
    assert (s.num_points, s.current) == (500, 451) and not s.need_new_kf(0.1)               # 49 > 50 ?
    s.erased(449)
    assert s.need_new_kf(0.1)                                                                # 51 > 50
    assert s.need_new_kf_image(0.1, 60, 80) and not s.need_new_kf_image(0.09, 60, 80)       # 449 < 480, 449 < 432 ?
    s.set_keyframe(300)
    assert (s.num_points, s.current) == (300, 300)
    t = kp.NumPoints()
    t.build_keyframe(10, 10)
    t.num_points = 5                            # more points than num_points: unsigned - size_t wraps, as in the reference
    assert t.need_new_kf(0.1)


def test_projection_identity_is_the_keyframe_pixel():
    case = kc.projection_cases()[0]
    inp = kc.projection_inputs(case, T7=np.array([0, 0, 0, 0, 0, 0, 1.0]))
    out = kp.project(**inp)
    assert np.abs(out["px"] - inp["kpix"][:, 0]).max() < 1e-11 and np.abs(out["py"] - inp["kpix"][:, 1]).max() < 1e-11
    assert np.abs(out["idp"] / inp["mu"] - 1.0).max() < 1e-14
    R = kp.quat_to_R([0.1, -0.3, 0.2, 0.9])
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(R) - 1.0) < 1e-15


@pytest.mark.parametrize("case", kc.projection_cases(), ids=lambda c: c[0])
def test_projection_cases_discriminate(case):
    inp = kc.projection_inputs(case)
    out = kp.project(**inp)
    dH, dW = inp["dst_size"]
    ok = out["Zp"] > 0
    px, py = out["px"], out["py"]
    sides = dict(left=(ok & (px < 0)).sum(), right=(ok & (px >= dW)).sum(), top=(ok & (py < 0)).sum(), bottom=(ok & (py >= dH)).sum())
    print(case[0], sides, "behind", int((~ok).sum()), "kept", float(out["keep"].mean()))
    assert all(v >= 3 for v in sides.values()), sides
    assert (~ok).sum() >= 3 and out["keep"].mean() >= 0.25
    fin = np.isfinite(px) & np.isfinite(py)
    edge = np.minimum.reduce([np.abs(px[fin]), np.abs(px[fin] - dW), np.abs(py[fin]), np.abs(py[fin] - dH)])
    assert edge.min() > 1e-6, edge.min()
    assert np.array_equal(out["src"], np.flatnonzero(out["keep"])) and len(out["xy"]) == out["keep"].sum()
    assert np.array_equal(kp.project(**inp, dtype=np.longdouble)["keep"], out["keep"])


def test_projection_behind_case_keeps_points_behind_the_camera():
    inp = kc.projection_inputs(kc.behind_case())
    out = kp.project(**inp)
    dH, dW = inp["dst_size"]
    behind = (out["Zp"] <= 0) & out["keep"]
    print("behind and kept", int(behind.sum()), "of", len(behind))
    assert behind.sum() >= 10 and (out["idp"][behind] < 0).all()
    px, py = out["px"], out["py"]
    assert np.minimum.reduce([np.abs(px), np.abs(px - dW), np.abs(py), np.abs(py - dH)]).min() > 1e-6
    assert np.array_equal(kp.project(**inp, dtype=np.longdouble)["keep"], out["keep"])


def test_projection_edge_exact_case():
    """px == dst_W and py == dst_H are out, px == 0 and py == 0 are in"""
    al, T7, K_dst, size, keep = kc.edge_exact_case()
    K = (al.fx, al.fy, al.cx, al.cy)
    out = kp.project(kp.slot_pixels(al.norm_coord, *K), sc.f32(al.idp), K, T7, K_dst, size)
    assert np.array_equal(out["px"], 100.0 * al.norm_coord[:, 0] + 25.0) and np.array_equal(out["py"], 80.0 * al.norm_coord[:, 1] + 20.0)
    assert (out["px"] == 75).sum() == 2 and (out["py"] == 40).sum() == 2 and (out["px"] == 0).sum() == 2 and (out["py"] == 0).sum() == 2
    assert np.array_equal(out["keep"], keep)


def test_projection_allowance():
    """the GPU test's tolerance: 4 x the oracle's own distance from extended precision.  Above 1e-9 px the cases would be ill-conditioned"""
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is no wider than double here"
    dxy, didp = kc.projection_allowance()
    print("projection allowance: %.3e px, %.3e relative" % (dxy, didp))
    assert 0.0 < dxy <= 1e-9 and 0.0 < didp <= 1e-12
