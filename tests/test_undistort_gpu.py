"""eds_und on the device against the numpy oracle of the reference (tests/np_undistort_oracle.py) AND against edsund:: compiled with g++
(tests/undistort_harness.py), bit for bit: K, the map, every plane, every exposure.  A NaN (a zero vignette entry under a raw 0) is
compared as NaN whatever its sign or payload.  Shapes are the smallest at which the kernels can go wrong — 40 x 32 to 36 x 28 and
37 x 29 to 37 x 29, no multiple of the 64 x 4 workgroup tile, with pixels at -1 and taps on the raw image's last row and column — plus
one 640 x 480 case for grid coverage."""
import importlib

import numpy as np
import pytest

import np_undistort_oracle as uo
import undistort_cases as uc
import undistort_harness as uh

capi = importlib.import_module("slam-eds_amd.capi")
und = importlib.import_module("slam-eds_amd.undistort")
pytestmark = pytest.mark.gpu
SCENARIOS = uc.scenarios()
ERR_INVALID = capi.ERR_INVALID


def make_dev(g, slots=1):
    return und.Undistorter(und.geometry(**g), slots)


def make_host(g, slots=1):
    return uh.HostUndistorter(und.geometry(**g), slots)


def all_planes(u):
    return np.stack([u.get_image(k) for k in range(u.slots)])


def check_scenario(sc, geometry=None):
    want = uc.expected(sc, geometry)
    host_planes, host_e, _ = uc.run_scenario(sc, make_host, geometry)
    assert uc.same_bits(host_planes, want["planes"]) and uc.same_bits(host_e, want["exposures"])
    planes, e, u = uc.run_scenario(sc, make_dev, geometry)
    assert u.form == und.FORM_AUTO
    su = want["setup"]
    assert np.array_equal(u.K, su["K"]) and uc.same_bits(u.map[0], su["mapx"]) and uc.same_bits(u.map[1], su["mapy"])
    assert u.passthrough == su["passthrough"]
    assert uc.same_bits(e, want["exposures"])
    assert uc.same_bits(planes, want["planes"]), np.argwhere(planes.view(np.uint32) != want["planes"].view(np.uint32))[:8]
    # fused against two-pass against the default that chooses by size, and each against its repetition
    g, raw, G, vig = uc.scenario_inputs(sc, geometry)
    for form in (und.FORM_FUSED, und.FORM_TWO_PASS, und.FORM_AUTO):
        u.form = form
        assert u.form == form
        for _ in range(2):
            e2 = u.process(raw, sc.exposures, factor=sc.factor)
            assert uc.same_bits(all_planes(u), want["planes"]) and uc.same_bits(e2, want["exposures"])
    return u, want


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_planes_equal_the_oracle_and_the_host(name):
    u, want = check_scenario(SCENARIOS[name])
    if name == "mode2_u8_batch_nan":
        assert np.isnan(want["planes"][0]).any() and want["branches"] == ["photometric", "plain", "photometric"]
    if name == "use_exposure_off_last_tap":
        mx, my = u.map
        assert ((mx.astype(int) == u.w_org - 2) & (my.astype(int) == u.h_org - 2) & (mx >= 0)).any()
    u.close()


def test_640x480_covers_the_grid():
    sc = uc._s("grid_mode2", None, exposures=(0.02, 0.0), factor=0.9, seed=21)
    u, want = check_scenario(sc, uc.grid_geometry())
    assert want["planes"].shape == (2, 480, 640) and want["branches"] == ["photometric", "plain"]
    u.close()


def test_the_default_form_on_both_sides_of_its_threshold():
    """EDS_UND_FORM_AUTO is the fused kernel below 4 Mi raw pixels a call and the two-pass form from there on: 13 and 14 frames of
    640 x 480 are 3 993 600 and 4 300 800"""
    geo = uc.grid_geometry()
    sc = uc._s("grid_14", None, exposures=(0.02,) * 13 + (0.0,), factor=0.9, seed=22)
    want = uc.expected(sc, geo)
    g, raw, G, vig = uc.scenario_inputs(sc, geo)
    assert 13 * raw[0].size < 4 << 20 <= 14 * raw[0].size
    u = make_dev(g, 14)
    u.set_photometric(G, vig)
    assert u.form == und.FORM_AUTO
    for n in (13, 14):
        u.process(raw[::-1].copy(), sc.exposures[::-1])                     # something else in every slot
        u.process(raw[:n], sc.exposures[:n], factor=sc.factor)
        assert uc.same_bits(all_planes(u)[:n], want["planes"][:n])
    with pytest.raises(capi.EdsError) as e:
        u.form = 3
    assert e.value.code == ERR_INVALID and u.form == und.FORM_AUTO
    u.close()


def test_pitched_host_input_and_device_input():
    sc = SCENARIOS["mode2_u8_batch_nan"]
    want = uc.expected(sc)
    g, raw, G, vig = uc.scenario_inputs(sc)
    n, h, w = raw.shape
    u = make_dev(g, n)
    u.set_photometric(G, vig)
    # host memory, rows 7 and frames 3 rows further apart than dense
    big = np.full((n, h + 3, w + 7), 201, np.uint8)
    big[:, :h, :w] = raw
    view = big[:, :h, :w]
    assert view.strides == ((h + 3) * (w + 7), w + 7, 1)
    u.process(view, sc.exposures, factor=sc.factor)
    assert uc.same_bits(all_planes(u), want["planes"])
    # device memory, dense
    d = capi.DeviceArray.from_numpy(raw)
    u.process(raw[::-1].copy(), sc.exposures, factor=sc.factor)            # something else in between
    assert not uc.same_bits(all_planes(u), want["planes"])
    u.process(d, sc.exposures, factor=sc.factor)
    assert uc.same_bits(all_planes(u), want["planes"])
    # device memory, pitched
    db = capi.DeviceArray.from_numpy(big)
    u.process(raw[::-1].copy(), sc.exposures, factor=sc.factor)
    u.process(db.view((n, h, w), big.strides), sc.exposures, factor=sc.factor)
    assert uc.same_bits(all_planes(u), want["planes"])
    # uint16 from the device
    sc16 = SCENARIOS["u16_g65536_rule"]
    want16 = uc.expected(sc16)
    g16, raw16, G16, vig16 = uc.scenario_inputs(sc16)
    u16 = make_dev(g16, 2)
    u16.set_photometric(G16, vig16)
    u16.process(capi.DeviceArray.from_numpy(raw16), sc16.exposures, factor=sc16.factor)
    assert uc.same_bits(all_planes(u16), want16["planes"])
    u.close()
    u16.close()


def test_first_slot_leaves_the_other_slots_alone():
    sc = SCENARIOS["mode2_u8_batch_nan"]
    want = uc.expected(sc)
    g, raw, G, vig = uc.scenario_inputs(sc)
    u = make_dev(g, 5)
    assert not all_planes(u).any()                                        # zeros before the first process
    u.set_photometric(G, vig)
    other = uc.raw_frames(5, g["h_org"], g["w_org"], 77)
    u.process(other, [0.01] * 5)
    before = all_planes(u)
    e = u.process(raw[1:], sc.exposures[1:], factor=sc.factor, first_slot=2)
    after = all_planes(u)
    assert uc.same_bits(after[2:4], want["planes"][1:]) and uc.same_bits(e, want["exposures"][1:])
    assert uc.same_bits(after[[0, 1, 4]], before[[0, 1, 4]]) and not uc.same_bits(after[2:4], before[2:4])
    u.close()


def test_a_caller_map():
    sc = SCENARIOS["given"]
    want = uc.expected(sc)
    g, raw, G, vig = uc.scenario_inputs(sc)
    rng = np.random.default_rng(8)
    cx = rng.uniform(0.01, g["w_org"] - 1.01, (g["h"], g["w"])).astype(np.float32)
    cy = rng.uniform(0.01, g["h_org"] - 1.01, (g["h"], g["w"])).astype(np.float32)
    cx[0, 0], cy[0, 0] = g["w_org"] - 1.5, g["h_org"] - 1.5               # the taps end on the raw image's last row and column
    cx[3, 5], cy[3, 5] = -1, -1
    ref = uo.undistort(want["setup"], want["photometric"], raw[0], sc.exposures[0], sc.factor, mapx=cx, mapy=cy)[0]
    assert ref[3, 5] == 0 and ref[0, 0] != 0
    for make in (make_host, make_dev):
        u = make(g, 1)
        u.set_photometric(G, vig)
        u.set_map(cx, cy)
        assert uc.same_bits(u.map[0], cx) and uc.same_bits(u.map[1], cy)
        u.process(raw, sc.exposures, factor=sc.factor)
        assert uc.same_bits(u.get_image(0), ref)
        u.close()
    # ... and on a passthrough handle the caller's map ends the passthrough
    scp = SCENARIOS["passthrough"]
    wantp = uc.expected(scp)
    gp, rawp, Gp, vigp = uc.scenario_inputs(scp)
    u = make_dev(gp, 1)
    u.set_photometric(Gp, vigp)
    assert u.passthrough
    px, py = cx[:gp["h"], :gp["w"]].copy(), cy[:gp["h"], :gp["w"]].copy()
    u.set_map(px, py)
    assert not u.passthrough
    u.process(rawp[0], [scp.exposures[0]], factor=scp.factor)
    refp = uo.undistort(wantp["setup"], wantp["photometric"], rawp[0], scp.exposures[0], scp.factor, mapx=px, mapy=py)[0]
    assert uc.same_bits(u.get_image(0), refp)
    u.close()


def _refused(call):
    with pytest.raises(capi.EdsError) as e:
        call()
    assert e.value.code == ERR_INVALID, e.value
    return e.value


def test_errors_leave_the_planes_as_they_were():
    sc = SCENARIOS["mode2_u8_batch_nan"]
    g, raw, G, vig = uc.scenario_inputs(sc)
    n, h, w = raw.shape
    u = make_dev(g, n)
    u.set_photometric(G, vig)
    u.process(raw, sc.exposures, factor=sc.factor)
    before, map_before = all_planes(u), u.map

    def unchanged():
        return uc.same_bits(all_planes(u), before) and uc.same_bits(u.map[0], map_before[0]) and uc.same_bits(u.map[1], map_before[1])

    other = np.ascontiguousarray(raw[::-1])
    # a host pointer handed over as device memory
    _refused(lambda: u.process((other.ctypes.data, other.shape, None, other.dtype), sc.exposures))
    assert unchanged()
    # a device range one frame short of what would be read
    short = capi.DeviceArray.from_numpy(other[:n - 1])
    _refused(lambda: u.process((short.ptr, other.shape, None, other.dtype), sc.exposures))
    assert unchanged()
    # ... and one byte short
    tight = capi.DeviceArray.from_numpy(other.reshape(-1)[:-1])
    _refused(lambda: u.process((tight.ptr, other.shape, None, other.dtype), sc.exposures))
    assert unchanged()
    # uint16 frames with a G table of 256 entries
    _refused(lambda: u.process(other.astype(np.uint16), sc.exposures))
    assert unchanged()
    # an invalid caller map: one pair on the raw image's last column
    bx, by = map_before[0].copy(), map_before[1].copy()
    bx[4, 4], by[4, 4] = g["w_org"] - 1.0, 3.0
    _refused(lambda: u.set_map(bx, by))
    by[4, 4] = np.nan
    _refused(lambda: u.set_map(bx, by))
    assert unchanged()
    # slots out of range
    _refused(lambda: u.process(other, sc.exposures, first_slot=1))
    _refused(lambda: u.process(other[:1], sc.exposures[:1], first_slot=n))
    _refused(lambda: u.process(other[:1], sc.exposures[:1], first_slot=-1))
    _refused(lambda: u.get_image(n))
    _refused(lambda: u.image(-1))
    assert unchanged()
    # the handle still works
    u.process(raw, sc.exposures, factor=sc.factor)
    assert uc.same_bits(all_planes(u), before)
    u.close()


def test_the_plane_is_handed_over_on_the_device():
    """eds_und_image into eds_sel_set_image and eds_ct_set_new with on_device = 1: their level 0 equals what the same handles build from
    the oracle's plane uploaded from the host"""
    select = importlib.import_module("slam-eds_amd.select")
    coarse = importlib.import_module("slam-eds_amd.coarse")
    sc = uc._s("handover", None, exposures=(0.02,), seed=31)
    geo = uc.handover_geometry()
    want = uc.expected(sc, geo)
    planes, _, u = uc.run_scenario(sc, make_dev, geo)
    assert uc.same_bits(planes, want["planes"])
    H, W = u.h, u.w
    view = u.image(0)
    assert capi.is_device_source(view) and capi.device_array_info(view)[1:] == ((H, W), (W, 1), np.dtype(np.float32))
    sel_dev, sel_host = select.Selector(H, W), select.Selector(H, W)
    sel_dev.set_image(view)
    sel_host.set_image(want["planes"][0])
    assert uc.same_bits(sel_dev.level(0), sel_host.level(0)) and np.ptp(sel_host.level(0)[..., 1]) > 0
    ct_dev, ct_host = coarse.CoarseTracker(H, W, levels=3), coarse.CoarseTracker(H, W, levels=3)
    K = u.K
    for ct in (ct_dev, ct_host):                # the calibration first: it is what puts the level shapes on the device
        ct.set_calib(K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    ct_dev.set_new(view, exposure=0.02)
    ct_host.set_new(want["planes"][0], exposure=0.02)
    assert uc.same_bits(ct_dev.level(coarse.NEW_IMAGE, 0), ct_host.level(coarse.NEW_IMAGE, 0))
    assert uc.same_bits(ct_host.level(coarse.NEW_IMAGE, 0)[..., 0], want["planes"][0])
    for x in (sel_dev, sel_host, ct_dev, ct_host, u):
        x.close()
