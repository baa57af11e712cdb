"""include/eds_hip_window.h on the device against csrc/eds_window.hpp under g++ (tests/window_harness.py), BIT FOR BIT (any NaN equal to
any NaN) on every case of tests/window_cases.py and every output of eds_win_get_residuals, eds_win_get_points, the energy, the counts, nres,
every accumulator word and H_A, b_A, H_sc, b_sc of eds_win_accumulate; the second linearize -> apply -> point_hessians round after eds_win_set_idepths; a run against its repetition; device-pointer
against host-pointer frames; the error codes, returned with nothing changed; and a frame against eds_ct_get_level and
eds_imm_get_image of the same image."""
import importlib

import numpy as np
import pytest

import window_cases as wc
import window_harness as wh

pytestmark = pytest.mark.gpu
NAMES = list(wc.cases())


@pytest.fixture(scope="module")
def window(capi, gpu):
    return importlib.import_module("slam-eds_amd.window")


def same_bits(a, b):
    """bit equality of two arrays, any NaN equal to any NaN"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == "f":
        ia, ib = a.view(f"u{a.dtype.itemsize}"), b.view(f"u{a.dtype.itemsize}")
        return bool(((ia == ib) | (np.isnan(a) & np.isnan(b))).all())
    return bool((a == b).all())


def same_rounds(got, want):
    """the first difference between two results of window_harness.run_rounds, or None"""
    for rnd, (g, w) in enumerate(zip(got, want)):
        for k in ("energy", "counts", "nres"):
            if not same_bits(g[k], w[k]):
                return rnd, k, g[k], w[k]
        if ("accumulated" in g) != ("accumulated" in w):
            return rnd, "accumulated", None
        for stage in ("linearized", "residuals", "points") + (("accumulated",) if "accumulated" in g else ()):
            for k in g[stage]:
                if not same_bits(g[stage][k], w[stage][k]):
                    return rnd, stage, k
    return None


def _device(window, c):
    return wh.open_case(c, cls=lambda H, W, F: window.Window(H, W, F, max_points=2048, max_residuals=8192))


@pytest.fixture(scope="module")
def host():
    """every case under g++, made once"""
    out = {}
    for name, c in wc.cases().items():
        w = wh.open_case(c)
        out[name] = dict(rounds=wh.run_rounds(w, c, accumulate=True), frames=[w.frame(f) for f in range(c.F)])
        w.close()
    return out


@pytest.mark.parametrize("name", NAMES)
def test_every_output_of_both_rounds_equals_the_host_restatement_bit_for_bit(window, host, name):
    c = wc.cases()[name]
    w = _device(window, c)
    for f in range(c.F):
        assert same_bits(w.frame(f), host[name]["frames"][f]), (name, f)
    got = wh.run_rounds(w, c, accumulate=True)              # H_A, b_A, H_sc, b_sc, every accumulator word and nres included
    assert same_rounds(got, host[name]["rounds"]) is None
    assert set(got[1]["accumulated"]) == {"H_A", "b_A", "H_sc", "b_sc", "acc", "nres"}
    assert got[0]["counts"].sum() == len(c.point)
    w.close()
    w2 = _device(window, c)                                     # a run equals its repetition
    assert same_rounds(wh.run_rounds(w2, c, accumulate=True), got) is None
    w2.close()


def test_apply_without_copy_equals_the_host(window):
    c = wc.cases()["f3_513"]
    w, h = _device(window, c), wh.open_case(c)
    assert same_rounds(wh.run_rounds(w, c, copy_jacobians=False), wh.run_rounds(h, c, copy_jacobians=False)) is None
    w.close()
    h.close()


def test_device_pointer_frames_equal_host_frames_and_errors_change_nothing(window, capi, host):
    c = wc.cases()["f3_5"]
    pad = np.full((c.F, c.H + 3, c.W + 5), 7.0, np.float32)
    pad[:, :c.H, :c.W] = c.images
    d = capi.DeviceArray.from_numpy(pad)
    row, frm = 4 * (c.W + 5), 4 * (c.W + 5) * (c.H + 3)
    w = window.Window(c.H, c.W, c.F, max_points=64, max_residuals=64)
    w.set_params(**c.prm)
    w.set_calib(*c.K)
    w.set_frames(0, d.view((c.F, c.H, c.W), (frm, row, 4)))
    w.set_points(c.host, c.uv, c.color, c.weights, c.ids, c.idz)
    w.set_residuals(c.point, c.target, c.state, c.energy)
    for f in range(c.F):
        assert same_bits(w.frame(f), host["f3_5"]["frames"][f])
    energy, counts = w.linearize(c.F, c.precalc, c.th)
    before = w.residuals()
    assert same_bits(np.float64(energy), host["f3_5"]["rounds"][0]["energy"])
    assert all(same_bits(before[k], host["f3_5"]["rounds"][0]["linearized"][k]) for k in before)
    w.apply(True)
    acc_before = w.accumulate(c.F, c.adH, c.adT, c.prior, c.delta, c.lf, bool(c.shift))
    before, pts_before = w.residuals(), w.points()                 # everything a refused call could have touched

    def refused(code, fn, *args, **kw):
        with pytest.raises(capi.EdsError) as e:
            fn(*args, **kw)
        assert e.value.code == code, e.value

    host_mem = np.ascontiguousarray(c.images[0])
    refused(capi.ERR_INVALID, w.set_frames, 0, (int(host_mem.ctypes.data), host_mem.shape, None, np.float32))      # a host pointer as device memory
    small = capi.DeviceArray.from_numpy(host_mem[:8])
    refused(capi.ERR_INVALID, w.set_frames, 0, (small.ptr, host_mem.shape, None, np.float32))                      # past its allocation
    refused(capi.ERR_INVALID, w.set_frames, c.F, c.images[0])                                                      # no such frame
    bad = c.precalc.copy()
    bad[1, 3] = np.nan
    refused(capi.ERR_INVALID, w.linearize, c.F, bad, c.th)
    refused(capi.ERR_INVALID, w.linearize, c.F, c.precalc, np.array([1.0, np.inf, 1.0]))
    refused(capi.ERR_INVALID, w.linearize, 2, c.precalc[:4], c.th[:2])                                             # a target is not below F
    refused(capi.ERR_INVALID, w.set_params, huber_th=0.0)
    refused(capi.ERR_INVALID, w.set_params, scale_f=float("nan"))
    refused(capi.ERR_INVALID, w.set_calib, 0.0, 50.0, 1.0, 1.0)
    refused(capi.ERR_INVALID, w.set_residuals, [0, 0], [c.host[0], 1])                                             # target == host
    refused(capi.ERR_INVALID, w.set_residuals, [1, 0], [1 - c.host[1] % 2, 1])                                     # not grouped by point
    refused(capi.ERR_INVALID, w.set_residuals, [len(c.host)], [1])
    refused(capi.ERR_INVALID, w.set_residuals, [0], [c.F])
    refused(capi.ERR_INVALID, w.set_residuals, [0], [1 if c.host[0] != 1 else 0], [3])
    refused(capi.ERR_INVALID, w.set_points, [0, 1, 0], np.zeros((3, 2)), np.zeros((3, 8)), np.zeros((3, 8)), np.ones(3))    # not grouped by host
    refused(capi.ERR_INVALID, w.set_points, [c.F], np.zeros((1, 2)), np.zeros((1, 8)), np.zeros((1, 8)), np.ones(1))
    refused(capi.ERR_INVALID, w.point_hessians, np.full(len(c.host), np.nan))
    bad_ad = c.adH.copy()
    bad_ad[2, 3, 3] = np.inf
    refused(capi.ERR_INVALID, w.accumulate, c.F, bad_ad, c.adT)
    refused(capi.ERR_INVALID, w.accumulate, c.F, c.adH, bad_ad)
    refused(capi.ERR_INVALID, w.accumulate, 2, c.adH[:4], c.adT[:4])                                               # a target is not below F
    refused(capi.ERR_INVALID, w.accumulate, c.F, c.adH, c.adT, np.full(len(c.host), np.inf))
    # every refusal left the state as it was
    after, pts_after = w.residuals(), w.points()
    assert all(same_bits(after[k], before[k]) for k in before) and all(same_bits(pts_after[k], pts_before[k]) for k in pts_before)
    acc_after = w.accumulate(c.F, c.adH, c.adT, c.prior, c.delta, c.lf, bool(c.shift))
    assert all(same_bits(acc_after[k], acc_before[k]) for k in acc_before)
    h = wh.open_case(c)                                            # the same calls on the host restatement
    h.linearize(c.F, c.precalc, c.th)
    h.apply(True)
    e2, c2 = w.linearize(c.F, c.precalc, c.th)
    e3, c3 = h.linearize(c.F, c.precalc, c.th)
    assert e2 == e3 and np.array_equal(c2, c3) and c2.sum() == counts.sum()
    h.close()
    w.close()
    for shape in ((4, 64, 8), (48, 64, 1), (48, 64, 9), (48, 64, 8, 0), (48, 64, 8, 1, 0)):
        with pytest.raises(capi.EdsError) as e:
            window.Window(*shape)
        assert e.value.code == capi.ERR_INVALID
    w = window.Window(c.H, c.W, c.F, max_points=64, max_residuals=64)
    refused(capi.ERR_STATE, w.apply)                                                                               # nothing linearized yet
    refused(capi.ERR_STATE, w.linearize, c.F, c.precalc, c.th)                                                     # no calibration
    w.set_calib(*c.K)
    refused(capi.ERR_STATE, w.linearize, c.F, c.precalc, c.th)                                                     # no frames
    refused(capi.ERR_STATE, w.frame, 0)
    w.set_frames(0, c.images[:2])
    refused(capi.ERR_STATE, w.linearize, c.F, c.precalc, c.th)                                                     # frame 2 is missing
    assert w.linearize(2, c.precalc[:4], c.th[:2])[0] == 0.0                                                       # the empty window
    w.close()


def test_a_frame_equals_level_0_of_the_coarse_tracker_and_the_immature_images(window):
    coarse = importlib.import_module("slam-eds_amd.coarse")
    imm = importlib.import_module("slam-eds_amd.immature")
    c = wc.cases()["f3_5"]
    w = window.Window(c.H, c.W, 2, max_points=1, max_residuals=1)
    w.set_frames(1, c.images[2])
    t = coarse.CoarseTracker(c.H, c.W, 1, max_points=8, max_tries=1)
    t.set_calib(*c.K)
    t.set_new(c.images[2])
    h = imm.ImmaturePoints(c.H, c.W, 1, 8, 1)
    h.set_host_images(0, c.images[2])
    assert np.isnan(w.frame(1)).any()
    assert same_bits(w.frame(1), t.level(coarse.NEW_IMAGE, 0)) and same_bits(w.frame(1), h.image(imm.HOST_IMAGE, 0))
    for x in (w, t, h):
        x.close()


def test_points_without_residuals_have_empty_runs_on_the_device(window):
    """eds_win_set_points empties the residual table on the device as well: point_hessians straight after it — on a fresh handle, and
    after an earlier, smaller table whose residuals were active — adds nothing, as the host restatement does"""
    small, big = wc.cases()["f3_5"], wc.cases()["f3_513"]
    w, h = window.Window(big.H, big.W, big.F, max_points=2048, max_residuals=8192), wh.HostWindow(big.H, big.W, big.F)
    for x in (w, h):
        x.set_calib(*big.K)
        x.set_frames(0, big.images)
        x.set_points(small.host, small.uv, small.color, small.weights, small.ids, small.idz)
        assert x.point_hessians(small.prior, small.delta, small.lf, True) == 0                  # a fresh handle: no residual table yet
    assert all(same_bits(w.points()[k], h.points()[k]) for k, _, _ in wh.POINT_FIELDS)
    for x in (w, h):
        x.set_residuals(small.point, small.target, small.state, small.energy)
        x.linearize(small.F, small.precalc, small.th)
        x.apply(True)
        assert x.point_hessians(small.prior, small.delta, small.lf, True) > 0                   # the old table has active residuals
        x.set_points(big.host, big.uv, big.color, big.weights, big.ids, big.idz)               # more points than before
        assert x.point_hessians(big.prior, big.delta, big.lf, False) == 0
    got, want = w.points(), h.points()
    assert all(same_bits(got[k], want[k]) for k, _, _ in wh.POINT_FIELDS)
    assert not got["nres"].any() and not got["HdiF"].any() and not got["Hdd_accAF"].any()
    assert w.linearize(big.F, big.precalc, big.th)[1].sum() == 0 and len(w.residuals()["state"]) == 0
    w.close()
    h.close()
