"""include/eds_hip_immdepth.h on the device, bit for bit against the route that existed before it — the selection read back, edsimd::
nearest on the host (tests/immdepth_harness.py), eds_imm_create_points(idepth, distance) on a second eds_imm — for the cases of
tests/immdepth_cases.py: every point field before and after one eds_imm_trace, alive, the counts and eds_imd_get_nearest; the tree
against edskd::build_tree and the path that built it; the hand-over from an eds_win without leaving the device,
with one wait per create call; and the error codes, each of which leaves the points and the map as they were."""
import ctypes as C
import importlib

import numpy as np
import pytest

import immdepth_cases as dc
import immdepth_harness as dh
import map_cases as mc
import np_immature_oracle as no

pytestmark = pytest.mark.gpu
capi = importlib.import_module("slam-eds_amd.capi")
immature = importlib.import_module("slam-eds_amd.immature")
immdepth = importlib.import_module("slam-eds_amd.immdepth")
select = importlib.import_module("slam-eds_amd.select")
window = importlib.import_module("slam-eds_amd.window")
mp = importlib.import_module("slam-eds_amd.map")
H, W = dc.H, dc.W
NAMES = sorted(dc.cases())
MAXP = 1200
INV, ST = capi.ERR_INVALID, capi.ERR_STATE


@pytest.fixture(scope="module")
def hl():
    return dh.load_harness()


@pytest.fixture(scope="module")
def sel(gpu):
    """one selector over the cases' image, its selection made once and read back once"""
    s = select.Selector(H, W, table=np.random.default_rng(5).integers(0, 256, H * W).astype(np.uint8))
    s.set_image(dc.image())
    s.make_maps(600.0, 1)
    uv, typ = s.selection()
    assert len(uv) > 100
    yield s, uv, typ
    s.close()


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind == "f":
        u = f"u{a.dtype.itemsize}"
        return bool(((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))).all())
    return bool((a == b).all())


def _state(ip):
    return dict(ip.get(0), **ip.points(0))


def _same_state(a, b):
    sa, sb = _state(a), _state(b)
    return [k for k in sa if not _bits(sa[k], sb[k])]


def _open(max_points=MAXP):
    ip = immature.ImmaturePoints(H, W, 1, max_points, 1)
    ip.set_host_images(0, dc.image())
    ip.set_target_images(0, np.roll(dc.image(), 2, axis=1))
    return ip


PRE = immature.precalc(np.array([[60.0, 0, W / 2], [0, 60.0, H / 2], [0, 0, 1]]), np.eye(3), [0.03, 0.01, 0.0])


def _existing_route(hl, b, c, uv, typ, scale):
    """what a caller did before: the list on the host, the tree and the walk on the host, four arrays uploaded"""
    if len(c.xy) == 0:
        return b.create_points(0, uv, typ), dict(index=np.full(len(uv), -1, np.int32), idepth=np.zeros(len(uv), np.float32), distance=np.zeros(len(uv)))
    nn = dh.nearest(hl, dh.tree_of(hl, c.xy, c.idp), uv, scale)
    return b.create_points(0, uv, typ, nn["idepth"], nn["distance"]), nn


def _check_equal(a, d, b, alive_a, counts, alive_b, nn):
    assert a.num_points(0) == b.num_points(0) == len(alive_b)
    assert np.array_equal(alive_a, alive_b)
    assert _same_state(a, b) == []
    got = d.nearest(0)
    for k in ("index", "idepth", "distance"):
        assert _bits(got[k], nn[k]), k
    st = a.get(0)["lastTraceStatus"]
    assert counts == (int((alive_a & (st == no.GOOD)).sum()), int((alive_a & (st == no.UNINITIALIZED)).sum()))
    assert d.info()["waits"] == 1
    sa, sb = a.trace(0, 0, *PRE), b.trace(0, 0, *PRE)
    assert np.array_equal(sa, sb) and _same_state(a, b) == []


@pytest.mark.parametrize("name", NAMES)
def test_selected_pixels_equal_the_existing_route(hl, sel, name):
    s, uv, typ = sel
    c = dc.cases()[name]
    a, b = _open(), _open()
    d = immdepth.ImmatureDepth(a)
    assert d.set_depth_map(c.xy, c.idp) == (not dh.device_builds(hl, c.xy) and len(c.xy) > 0)
    alive_a, counts = d.create_points_selected(0, s, scale=c.scale)
    assert d.info()["waits"] == 1
    keep = (uv[:, 0] >= 3) & (uv[:, 0] <= W - 5) & (uv[:, 1] >= 3) & (uv[:, 1] <= H - 5)
    assert 50 < keep.sum() < len(uv)
    alive_b, nn = _existing_route(hl, b, c, uv[keep], typ[keep], c.scale)
    _check_equal(a, d, b, alive_a, counts, alive_b, nn)
    if name == "empty":                                   # ... and that is eds_imm_create_points_selected, bit for bit
        e = _open()
        assert np.array_equal(e.create_points_selected(0, s), alive_a)
        e.trace(0, 0, *PRE)
        assert _same_state(e, a) == []
        e.close()
    a.close(); b.close()


@pytest.mark.parametrize("name", NAMES)
def test_the_cases_own_pixels_equal_the_existing_route(hl, gpu, name):
    """the cases' lists hold what the selection rectangle never passes: border pixels, whose pattern leaves the image"""
    c = dc.cases()[name]
    a, b = _open(), _open()
    d = immdepth.ImmatureDepth(a)
    d.set_depth_map(c.xy, c.idp)
    alive_a, counts = d.create_points(0, c.uv, c.type, scale=c.scale)
    alive_b, nn = _existing_route(hl, b, c, c.uv, c.type, c.scale)
    assert name == "distance_one" or not alive_b.all()
    _check_equal(a, d, b, alive_a, counts, alive_b, nn)
    a.close(); b.close()


@pytest.mark.parametrize("n", dc.LIST_SIZES)
@pytest.mark.parametrize("on_device", (False, True))
def test_list_sizes_in_host_and_device_memory(hl, gpu, n, on_device):
    c = dc.cases()["random_1000"]
    uv, typ = dc.pixels(n, 900 + n)
    a, b = _open(), _open()
    d = immdepth.ImmatureDepth(a)
    d.set_depth_map(c.xy, c.idp)
    if on_device:
        duv, dtyp = capi.DeviceArray.from_numpy(uv), capi.DeviceArray.from_numpy(typ)
        alive_a, counts = d.create_points(0, duv, dtyp)
    else:
        alive_a, counts = d.create_points(0, uv, typ)
    assert d.info()["waits"] == 1
    alive_b, nn = _existing_route(hl, b, c, uv, typ, None)
    _check_equal(a, d, b, alive_a, counts, alive_b, nn)
    a.close(); b.close()


@pytest.mark.parametrize("name", NAMES)
def test_tree_and_the_path_that_built_it(hl, gpu, name):
    c = dc.cases()[name]
    a = _open(8)
    d = immdepth.ImmatureDepth(a)
    on_host = d.set_depth_map(capi.DeviceArray.from_numpy(c.xy), capi.DeviceArray.from_numpy(c.idp)) if len(c.xy) else d.set_depth_map(c.xy, c.idp)
    if name.startswith("random_"):
        assert on_host == (len(c.xy) > 4096)
    if name in ("grid", "random_4097"):
        assert on_host
    assert on_host == (len(c.xy) > 0 and not dh.device_builds(hl, c.xy)) and d.info()["tree_on_host"] == int(on_host)
    perm, txy, tidp = dh.tree_of(hl, c.xy, c.idp)
    t = d.tree()
    assert np.array_equal(t["perm"], perm) and _bits(t["txy"], txy.reshape(-1, 2)) and _bits(t["tidp"], tidp)
    a.close()


def test_hand_over_from_the_window_without_leaving_the_device(hl, sel):
    s, uv, typ = sel
    rng = np.random.default_rng(77)
    per = [150, 170]
    n = sum(per)
    # a window whose field of view covers the new keyframe's and more, under real-valued poses: the map is unambiguous
    c = dict(host=np.repeat(np.arange(2), per).astype(np.int32), ids=rng.uniform(0.4, 1.6, n).astype(np.float32),
             uv=np.stack([rng.uniform(2, 92, n), rng.uniform(2, 68, n)], axis=1).astype(np.float32), calib=np.array([70.2, 69.1, 47.3, 35.4], np.float32),
             T_w_c=np.stack([mc.random_pose(rng, 0.05, 0.1) for _ in range(2)]))
    T_kf_w = mc.inverse(mc.random_pose(rng, 0.06, 0.1))
    K = np.array([52.0, 51.0, 31.2, 23.4])
    w = window.Window(72, 96, 8, max_points=n, max_residuals=1)
    w.set_calib(*[float(v) for v in c["calib"]])
    w.set_points(c["host"], c["uv"], np.zeros((n, 8), np.float32), np.ones((n, 8), np.float32), c["ids"], c["ids"])
    a, b = _open(), _open()
    da, db = immdepth.ImmatureDepth(a), immdepth.ImmatureDepth(b)
    alive_a, counts_a, maps, on_host = mp.seed_immature_from_window(da, 0, s, w, c["T_w_c"], T_kf_w, K, H, W)
    assert capi.is_device_array(maps["depth_xy"]) and 50 < maps["n"][0] < n and not on_host
    assert da.info()["waits"] == 1 and da.info()["map_n"] == maps["n"][0]
    # the same maps taken through the host
    hm = mp.window_depth_maps(w, c["T_w_c"], [T_kf_w], K.reshape(1, 4), H, W, src_index=False)
    m = int(hm["n"][0])
    assert m == maps["n"][0]
    assert not db.set_depth_map(hm["depth_xy"][0, :m], hm["depth_idp"][0, :m])
    alive_b, counts_b = db.create_points_selected(0, s)
    assert np.array_equal(alive_a, alive_b) and counts_a == counts_b and counts_a[0] > 0 and counts_a[1] > 0
    assert _same_state(a, b) == [] and all(_bits(da.nearest(0)[k], db.nearest(0)[k]) for k in ("index", "idepth", "distance"))
    ta, tb = da.tree(), db.tree()
    assert all(_bits(ta[k], tb[k]) for k in ta)
    # ... and through the existing route
    e = _open()
    keep = (uv[:, 0] >= 3) & (uv[:, 0] <= W - 5) & (uv[:, 1] >= 3) & (uv[:, 1] <= H - 5)
    nn = dh.nearest(hl, dh.tree_of(hl, hm["depth_xy"][0, :m], hm["depth_idp"][0, :m]), uv[keep])
    assert np.array_equal(e.create_points(0, uv[keep], typ[keep], nn["idepth"], nn["distance"]), alive_a) and _same_state(a, e) == []
    for h in (a, b, e, w):
        h.close()


def test_refused_calls_change_nothing(hl, sel):
    s, uv, typ = sel
    L = immdepth._lib()
    c = dc.cases()["random_65"]
    vp = capi.vp
    a = _open()
    d = immdepth.ImmatureDepth(a)
    rect = (3, 3, W - 5, H - 5)
    n_out = C.c_int(-7)
    sel_call = lambda imm, host, sh, r=rect: L.eds_imd_create_points_selected(imm, host, sh, *r, None, None, C.byref(n_out), None)
    a.create_points(0, [[20, 20], [30, 30]])
    before = _state(a)
    assert sel_call(a._h, 0, s._h) == ST                                                   # no map
    assert L.eds_imd_create_points(a._h, 0, 2, vp(c.uv), vp(c.type), 0, None, None, None) == ST
    assert L.eds_imd_get_tree(a._h, None, None, None) == ST
    d.set_depth_map(c.xy, c.idp)
    tree0, info0 = d.tree(), d.info()
    noimg = immature.ImmaturePoints(H, W, 2, 16, 1)
    noimg.set_host_images(0, dc.image())
    dn = immdepth.ImmatureDepth(noimg)
    dn.set_depth_map(c.xy, c.idp)
    assert sel_call(noimg._h, 1, s._h) == ST                                               # no host image
    assert L.eds_imd_get_nearest(noimg._h, 0, None, None, None) == ST                      # no create call on that host yet
    fresh = select.Selector(H, W, table=np.zeros(H * W, np.uint8))
    assert sel_call(a._h, 0, fresh._h) == ST                                               # no selection
    stale = select.Selector(H, W, table=np.zeros(H * W, np.uint8))
    stale.set_image(dc.image())
    stale.make_maps(600.0, 0)
    stale.set_image(dc.image()[::-1].copy())
    assert sel_call(a._h, 0, stale._h) == ST                                               # a stale selection
    other = select.Selector(H + 32, W, table=np.zeros((H + 32) * W, np.uint8))
    other.set_image(np.zeros((H + 32, W), np.float32))
    other.make_maps(10.0, 0)
    bad_xy, bad_idp = c.xy.copy(), c.idp.copy()
    bad_xy[7, 1] = np.inf
    nan_xy = c.xy.copy()
    nan_xy[0, 0] = np.nan
    dbad, dnan, didp = capi.DeviceArray.from_numpy(bad_xy), capi.DeviceArray.from_numpy(nan_xy), capi.DeviceArray.from_numpy(bad_idp)
    big_uv, big_typ = dc.pixels(MAXP + 1, 3)
    inf_scale = np.array([1.0, np.inf])
    bad = [
        sel_call(None, 0, s._h), sel_call(a._h, 0, None), sel_call(a._h, 1, s._h), sel_call(a._h, -1, s._h),
        sel_call(a._h, 0, other._h),                                                       # a selector of another size
        sel_call(a._h, 0, s._h, (3, 3, W, H - 5)), sel_call(a._h, 0, s._h, (-1, 3, W - 5, H - 5)), sel_call(a._h, 0, s._h, (30, 3, 20, H - 5)),
        L.eds_imd_create_points_selected(a._h, 0, s._h, *rect, vp(inf_scale), None, None, None),
        L.eds_imd_create_points(a._h, 0, 3, vp(c.uv), vp(c.type), 1, None, None, None),    # host pointers passed as device pointers
        L.eds_imd_create_points(a._h, 0, 3, None, vp(c.type), 0, None, None, None),
        L.eds_imd_create_points(a._h, 0, 3, vp(c.uv), vp(c.type), 2, None, None, None),
        L.eds_imd_create_points(a._h, 0, MAXP + 1, vp(big_uv), vp(big_typ), 0, None, None, None),     # more than max_points_per_host
        L.eds_imd_create_points(a._h, 0, -1, vp(c.uv), vp(c.type), 0, None, None, None),
        L.eds_imd_set_depth_map(a._h, 65, vp(c.xy), vp(c.idp), 1, None),                   # a host pointer passed as a device pointer
        L.eds_imd_set_depth_map(a._h, 65, vp(bad_xy), vp(c.idp), 0, None),                 # a non-finite coordinate in host memory ...
        L.eds_imd_set_depth_map(a._h, 65, vp(nan_xy), vp(c.idp), 0, None),
        L.eds_imd_set_depth_map(a._h, 65, C.c_void_p(dbad.ptr), C.c_void_p(didp.ptr), 1, None),      # ... and in device memory
        L.eds_imd_set_depth_map(a._h, 65, C.c_void_p(dnan.ptr), C.c_void_p(didp.ptr), 1, None),
        L.eds_imd_set_depth_map(a._h, -1, vp(c.xy), vp(c.idp), 0, None),
        L.eds_imd_set_depth_map(a._h, 65, None, vp(c.idp), 0, None),
        L.eds_imd_set_depth_map(a._h, 65, vp(c.xy), vp(c.idp), 3, None),
        L.eds_imd_set_depth_map(None, 65, vp(c.xy), vp(c.idp), 0, None),
        L.eds_imd_set_debug(a._h, 2), L.eds_imd_get_info(a._h, None), L.eds_imd_get_nearest(a._h, 4, None, None, None),
    ]
    assert bad == [INV] * len(bad), bad
    assert n_out.value == -7
    # the selection holds more pixels than a small handle: found on the device, reported by the one wait, nothing stored
    small = immature.ImmaturePoints(H, W, 1, 3, 1)
    small.set_host_images(0, dc.image())
    ds = immdepth.ImmatureDepth(small)
    ds.set_depth_map(c.xy, c.idp)
    small.create_points(0, [[20, 20], [30, 30]])
    small_before = _state(small)
    assert L.eds_imd_create_points_selected(small._h, 0, s._h, 0, 0, W - 1, H - 1, None, None, C.byref(n_out), None) == INV and n_out.value == -7
    assert small.num_points(0) == 2 and all(_bits(small_before[k], _state(small)[k]) for k in small_before)
    assert ds.create_points_selected(0, s, rect=(20, 20, 21, 20))[0].size <= 2             # ... and a rectangle that fits is taken
    # the points, the map and its tree are what they were
    assert a.num_points(0) == 2 and all(_bits(before[k], _state(a)[k]) for k in before)
    tree1, info1 = d.tree(), d.info()
    assert all(_bits(tree0[k], tree1[k]) for k in tree0) and info0["map_n"] == info1["map_n"] == 65 and info1["map_set"] == 1
    alive, _ = d.create_points(0, c.uv, c.type)
    assert len(alive) == len(c.uv)
    for h in (a, noimg, small, fresh, stale, other):
        h.close()
