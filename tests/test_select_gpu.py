"""include/eds_hip_select.h on the device against the literal numpy oracle (tests/np_select_oracle.py) and against edspix under g++
(tests/select_harness.py), bit for bit, on the committed cases of tests/select_cases.py: the three levels with absSquaredGrad, ths and
thsSmoothed, the map after every pass, n2 / n3 / n4, the potentials, numHaveSub and the selection list; device-memory and pitched
images, a run against its repetition, the kept histograms, the levels against eds_ct and eds_imm, eds_imm_create_points_selected against
eds_imm_create_points on the read-back list, and the error codes, each of which leaves the state as it was."""
import ctypes as C
import importlib

import numpy as np
import pytest

import np_select_oracle as so
import select_cases as sc
import select_harness as sh
from test_select_oracle import assert_equals_oracle, oracle_run, run_selector

pytestmark = pytest.mark.gpu
CASES = sc.cases()


@pytest.fixture(scope="module")
def sel(capi, gpu):
    return importlib.import_module("slam-eds_amd.select")


@pytest.fixture(scope="module")
def imm(capi, gpu):
    return importlib.import_module("slam-eds_amd.immature")


def _open(sel, c):
    return sel.Selector(c.H, c.W, table=c.table, **c.prm)


def _same(a, b):
    return all(np.array_equal(np.asarray(a[k]).view(np.uint32) if np.asarray(a[k]).dtype == np.float32 else a[k],
                              np.asarray(b[k]).view(np.uint32) if np.asarray(b[k]).dtype == np.float32 else b[k])
               for k in ("map", "uv", "type", "ths", "ths_s")) and a["passes"] == b["passes"] and a["num_have_sub"] == b["num_have_sub"] and \
        a["potential"] == b["potential"] and all(np.array_equal(x, y) for x, y in zip(a["pass_maps"], b["pass_maps"])) and \
        all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a["levels"], b["levels"]))


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_the_oracle_and_edspix(sel, name):
    c = CASES[name]
    s = _open(sel, c)
    got = run_selector(s, c)
    assert_equals_oracle(got, name)
    h = sh.HostSelector(c.H, c.W, c.table, **c.prm)
    assert _same(got, run_selector(h, c))
    assert s.scan_info() == h.scan_info()
    # the same image again: makeHists is skipped, and the result is makeMaps from the potential the first call left
    n2 = s.make_maps(c.density, c.recursions, c.th_factor)
    assert n2 == h.make_maps(c.density, c.recursions, c.th_factor)
    assert np.array_equal(s.map(), h.map()) and s.passes == h.passes and s.potential == h.potential
    s.close()


def test_ambiguous_cells_are_resolved_on_the_device(sel):
    for name in ("h_ramp_all_sensitive", "v_ramp_all_sensitive", "half_ramp_some_sensitive"):
        c = CASES[name]
        s = _open(sel, c)
        s.potential = c.potential
        s.set_image(c.image, c.B)
        s.make_maps(c.density, 0, c.th_factor)
        amb, n2_certain = s.scan_info()
        assert amb > 0 and s.passes[0][1] != n2_certain and s.passes[0][1] == oracle_run(name)[0]["passes"][0][1]
        s.close()


def test_device_pitched_and_repeated_runs_are_equal(sel, capi):
    c = CASES["odd_70x100_p1_ref"]
    a, b, p, d = (_open(sel, c) for _ in range(4))
    ra = run_selector(a, c)
    assert _same(ra, run_selector(b, c))                                    # a run equals its repetition
    wide = np.full((c.H, c.W + 9), np.float32(np.nan))
    wide[:, :c.W] = c.image
    cp = SimpleCase(c, wide[:, :c.W])                                        # host memory, rows W + 9 apart
    assert _same(ra, run_selector(p, cp))
    dev = capi.DeviceArray.from_numpy(wide)
    cd = SimpleCase(c, dev.view((c.H, c.W), (4 * (c.W + 9), 4)))             # device memory, pitched
    assert _same(ra, run_selector(d, cd))
    dense = capi.DeviceArray.from_numpy(c.image)
    b.potential = c.potential
    assert _same(ra, run_selector(b, SimpleCase(c, dense)))                  # device memory, dense; and the same object again
    for s in (a, b, p, d):
        s.close()


class SimpleCase:
    """a case with another image object"""

    def __init__(self, c, image):
        self.__dict__.update(c.__dict__)
        self.image = image


def test_a_new_image_histograms_again(sel):
    c, e = CASES["tex_64x96_sub"], CASES["tex_64x96_nodist"]
    s = _open(sel, c)
    run_selector(s, c)
    first = s.thresholds(sel.THS)
    s.potential = c.potential
    s.set_image(e.image)
    s.make_maps(c.density, c.recursions, c.th_factor)
    o = so.Selector(c.H, c.W, c.table, **c.prm)
    o.potential = c.potential
    o.set_image(e.image)
    r = o.make_maps(c.density, c.recursions, c.th_factor)
    assert np.array_equal(s.thresholds(sel.THS), o.ths) and not np.array_equal(first, o.ths)
    assert np.array_equal(s.map(), r["map"]) and s.passes == r["passes"]
    s.close()


def test_levels_equal_the_coarse_trackers_and_the_immature_points(sel, imm):
    coarse = importlib.import_module("slam-eds_amd.coarse")
    c = CASES["tex_96x64_keep_th2_B"]
    s = _open(sel, c)
    s.set_image(c.image, c.B)
    ct = coarse.CoarseTracker(c.H, c.W, levels=3, max_points=16)
    ct.set_calib(80.0, 80.0, c.W / 2, c.H / 2)                                # eds_ct uploads its geometry with the calibration
    ct.set_new(c.image)
    for lvl in range(3):
        assert np.array_equal(s.level(lvl)[:, :, :3].view(np.uint32), ct.level(coarse.NEW_IMAGE, lvl).view(np.uint32)), lvl
    ip = imm.ImmaturePoints(c.H, c.W, 1, 16, 1)
    ip.set_host_images(0, c.image)
    assert np.array_equal(s.level(0)[:, :, :3].view(np.uint32), ip.image(imm.HOST_IMAGE, 0).view(np.uint32))
    for h in (s, ct, ip):
        h.close()


def _points_state(ip):
    return dict(ip.get(0), **ip.points(0))


def test_create_points_selected_equals_create_points_on_the_read_back_list(sel, imm):
    import np_immature_oracle as no
    c = CASES["odd_70x100_p5_more"]
    s = _open(sel, c)
    run_selector(s, c)
    uv, typ = s.selection()
    rects = [None, (10, 20, 40, 70), (0, 0, c.W - 1, c.H - 1), (5, 5, 5, 5)]
    target = sc.texture(c.H, c.W, 14, amp=60.0)
    K = np.array([[80.0, 0, c.W / 2], [0, 80.0, c.H / 2], [0, 0, 1]])
    pre = imm.precalc(K, np.eye(3), [0.02, 0.01, 0.0])
    for rect in rects:
        x0, y0, x1, y1 = (3, 3, c.W - 5, c.H - 5) if rect is None else rect
        keep = (uv[:, 0] >= x0) & (uv[:, 0] <= x1) & (uv[:, 1] >= y0) & (uv[:, 1] <= y1)
        a, b = (imm.ImmaturePoints(c.H, c.W, 1, len(uv) + 1, 1) for _ in range(2))
        for ip in (a, b):
            ip.set_host_images(0, c.image)
            ip.set_target_images(0, target)
        alive_a = a.create_points_selected(0, s, rect)
        alive_b = b.create_points(0, uv[keep], typ[keep])
        assert a.num_points(0) == b.num_points(0) == int(keep.sum())
        assert np.array_equal(alive_a, alive_b)
        if rect is None:
            assert keep.sum() > 50 and not keep.all()
        sa, sb = _points_state(a), _points_state(b)
        assert all(no.same_bits(sa[k], sb[k]).all() for k in sa)
        ta, tb = a.trace(0, [0], *pre), b.trace(0, [0], *pre)                # a following trace is the same on both routes
        assert np.array_equal(ta, tb)
        sa, sb = _points_state(a), _points_state(b)
        assert all(no.same_bits(sa[k], sb[k]).all() for k in sa)
        a.close(), b.close()
    s.close()


def test_every_error_leaves_the_state_as_it_was(sel, imm, capi):
    L = capi.lib()
    c = CASES["tex_64x96_sub"]
    s = sel.Selector(c.H, c.W)
    n, npass = C.c_int(), C.c_int()
    img = np.ascontiguousarray(c.image)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.eds_sel_make_maps(s._h, 100.0, 1, 1.0, C.byref(n), None, 0, C.byref(npass), None) == capi.ERR_STATE      # no table
    s.set_random_pattern(c.table)
    assert L.eds_sel_make_maps(s._h, 100.0, 1, 1.0, C.byref(n), None, 0, C.byref(npass), None) == capi.ERR_STATE      # no image
    assert L.eds_sel_get_map(s._h, vp(np.zeros(c.H * c.W, np.uint8))) == capi.ERR_STATE
    ip = imm.ImmaturePoints(c.H, c.W, 1, 4000, 1)
    ip.set_host_images(0, c.image)
    ip.create_points(0, [[20, 20], [30, 30]])
    before_pts = _points_state(ip)
    assert L.eds_imm_create_points_selected(ip._h, 0, s._h, 3, 3, c.W - 5, c.H - 5, None, None) == capi.ERR_STATE     # no selection yet
    run_selector(s, c)
    state = lambda: (s.map().copy(), s.potential, s.selection(), s.passes)
    m0, p0, (uv0, t0), _ = state()
    bad = [
        L.eds_sel_set_image(s._h, None, 0, 0, None),
        L.eds_sel_set_image(s._h, vp(img), 0, 1, None),                          # a host pointer passed as device memory
        L.eds_sel_set_image(s._h, vp(img), c.W - 1, 0, None),
        L.eds_sel_set_image(s._h, vp(img), 0, 0, vp(np.full(256, np.nan, np.float32))),
        L.eds_sel_set_random_pattern(s._h, None, c.H * c.W),
        L.eds_sel_set_random_pattern(s._h, vp(c.table), c.H * c.W - 1),
        L.eds_sel_make_maps(s._h, 100.0, 1, 1.0, None, None, 0, None, None),
        L.eds_sel_make_maps(s._h, 0.0, 1, 1.0, C.byref(n), None, 0, None, None),
        L.eds_sel_make_maps(s._h, float("nan"), 1, 1.0, C.byref(n), None, 0, None, None),
        L.eds_sel_make_maps(s._h, 100.0, -1, 1.0, C.byref(n), None, 0, None, None),
        L.eds_sel_make_maps(s._h, 100.0, 1, float("inf"), C.byref(n), None, 0, None, None),
        L.eds_sel_make_maps(s._h, 100.0, 1, 1.0, C.byref(n), None, 2, None, None),
        L.eds_sel_set_potential(s._h, 0),
        L.eds_sel_get_map(s._h, None),
        L.eds_sel_get_selection(s._h, None, None, None),
        L.eds_sel_get_level(s._h, 3, vp(np.zeros(4, np.float32))),
        L.eds_sel_get_thresholds(s._h, 2, vp(np.zeros(4, np.float32))),
    ]
    assert bad == [capi.ERR_INVALID] * len(bad), bad
    with pytest.raises(capi.EdsError):
        s.set_params(min_grad_hist_cut=float("nan"))
    with pytest.raises(capi.EdsError):
        s.set_params(min_grad_hist_cut=1.5)
    other = sel.Selector(c.H + 32, c.W, table=np.zeros((c.H + 32) * c.W, np.uint8))
    other.set_image(np.zeros((c.H + 32, c.W), np.float32))
    other.make_maps(10.0, 0)
    bad = [
        L.eds_imm_create_points_selected(ip._h, 0, None, 3, 3, c.W - 5, c.H - 5, None, None),
        L.eds_imm_create_points_selected(None, 0, s._h, 3, 3, c.W - 5, c.H - 5, None, None),
        L.eds_imm_create_points_selected(ip._h, 0, other._h, 3, 3, c.W - 5, c.H - 5, None, None),    # mismatched imm / sel
        L.eds_imm_create_points_selected(ip._h, 1, s._h, 3, 3, c.W - 5, c.H - 5, None, None),
        L.eds_imm_create_points_selected(ip._h, 0, s._h, 3, 3, c.W, c.H - 5, None, None),            # a rectangle outside the image
        L.eds_imm_create_points_selected(ip._h, 0, s._h, -1, 3, c.W - 5, c.H - 5, None, None),
        L.eds_imm_create_points_selected(ip._h, 0, s._h, 30, 3, 20, c.H - 5, None, None),
    ]
    assert bad == [capi.ERR_INVALID] * len(bad), bad
    small = imm.ImmaturePoints(c.H, c.W, 1, 3, 1)
    small.set_host_images(0, c.image)
    assert L.eds_imm_create_points_selected(small._h, 0, s._h, 0, 0, c.W - 1, c.H - 1, None, None) == capi.ERR_INVALID   # more than it holds
    assert small.num_points(0) == 0
    m1, p1, (uv1, t1), _ = state()
    assert np.array_equal(m0, m1) and p0 == p1 and np.array_equal(uv0, uv1) and np.array_equal(t0, t1)
    assert ip.num_points(0) == 2
    after_pts = _points_state(ip)
    assert all(np.array_equal(before_pts[k], after_pts[k], equal_nan=True) for k in before_pts)
    assert_equals_oracle(dict(run_selector(_open(sel, c), c)), "tex_64x96_sub")
    for h in (s, other, ip, small):
        h.close()
