"""include/eds_hip_map.h on the device against csrc/eds_map.hpp under g++ (tests/map_harness.py) and the numpy restatement of the reference
(tests/np_map_oracle.py): bit for bit, as integer views, NaNs included — everything is correctly rounded IEEE fp32 / fp64 in one stated
order, so no tolerance is needed or allowed.
  1  the window's cloud, both fans, into host and into device memory, twice;
  2  the depth maps: batches against their singles, strides, the inlier rule's edges, degenerate inverse depths, Z' <= 0;
  3  the immature cloud: every lastTraceStatus, idepth_max NaN, negative and zero midpoints, dead points, a cap one too small;
  4  the cloud follows the tables: after eds_wsv_step_idepths, eds_wed_remove_points and eds_wed_insert_activated;
  5  the hand-over: window_depth_maps(device) -> eds_kfs_build_keyframes_dev against the oracle's maps -> eds_kfs_build_keyframes;
  6  a slot's cloud, seeded and unseeded, a sub-range, a batch in flight, a slot without a keyframe;
  7  refused calls: the code, and outputs that were not touched."""
import ctypes as C
import importlib

import numpy as np
import pytest

import kdbuild_cases as kc
import map_cases as mc
import map_harness as mh
import np_map_oracle as mo
import winedit_cases as wec
import winedit_harness as weh
import winsolve_harness as wsh

pytestmark = pytest.mark.gpu
capi = importlib.import_module("slam-eds_amd.capi")
window = importlib.import_module("slam-eds_amd.window")
winsolve = importlib.import_module("slam-eds_amd.winsolve")
winedit = importlib.import_module("slam-eds_amd.winedit")
immature = importlib.import_module("slam-eds_amd.immature")
mp = importlib.import_module("slam-eds_amd.map")
INV, ST = capi.ERR_INVALID, capi.ERR_STATE


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(mo.bits(a), mo.bits(b))


def code(call, *a, **kw):
    try:
        call(*a, **kw)
    except capi.EdsError as e:
        return e.code
    return capi.EDS_OK


def open_window(c, H=mc.WIN_H, W=mc.WIN_W, calib=True):
    n = len(c["host"])
    w = window.Window(H, W, 8, max_points=max(n, 1), max_residuals=1)
    if calib:
        w.set_calib(*[float(v) for v in c["calib"]])
    w.set_points(c["host"], c["uv"], np.zeros((n, 8), np.float32), np.ones((n, 8), np.float32), c["ids"], c["ids"])
    return w


def win_args(c):
    return c["host"], c["uv"], c["ids"], c["calib"], c["T_w_c"], c["mask"]


@pytest.fixture(scope="module")
def cases(gpu):
    edge, _ = mc.edge_case()
    return mc.window_cases(mh.chunk()) + [mc.degenerate_case(), mc.plane_case(), edge]


@pytest.fixture(scope="module")
def refs(cases):
    """the oracle's results, computed once: per case name dict(cloud={single: (points, per_host)}, maps=[...])"""
    out = {}
    for c in cases:
        out[c["name"]] = dict(cloud={s: mo.window_cloud(*win_args(c), s) for s in (True, False)},
                              maps=mo.window_depth_maps(*win_args(c), c["T_dst_w"], c["K_dst"], c["dst_H"], c["dst_W"]))
    return out


# -- 1. the window's cloud -------------------------------------------------------------------------------------------------------------------

def test_window_cloud_equals_host_restatement_and_oracle(cases, refs):
    for c in cases:
        w = open_window(c)
        for single in (True, False):
            ref, per_ref = refs[c["name"]]["cloud"][single]
            host_form, _ = mh.window_cloud(*win_args(c), single)
            got, per = mp.window_cloud(w, c["T_w_c"], c["mask"], single)
            assert same(got, ref) and same(got, host_form) and np.array_equal(per, per_ref), (c["name"], single)
            dev, per_d = mp.window_cloud(w, c["T_w_c"], c["mask"], single, device="array")
            assert same(dev.numpy()[:len(ref)], ref) and np.array_equal(per_d, per_ref), (c["name"], single)
            again, _ = mp.window_cloud(w, c["T_w_c"], c["mask"], single)                       # a run repeats exactly
            assert got.tobytes() == again.tobytes()
        w.close()


def test_the_large_window_crosses_many_sweeps(cases):
    big = [c for c in cases if c["name"] == "n20000"][0]
    assert mc.selected(big) == 20000 and 20000 > 16 * mh.chunk()


# -- 2. the depth maps -------------------------------------------------------------------------------------------------------------------------

def _maps(w, c, device, sl=slice(None), stride=None):
    r = mp.window_depth_maps(w, c["T_w_c"], c["T_dst_w"][sl], c["K_dst"][sl], c["dst_H"], c["dst_W"], c["mask"], stride=stride, device=device)
    get = (lambda a: a.numpy()) if device else (lambda a: a)
    xy, idp, src = get(r["depth_xy"]), get(r["depth_idp"]), get(r["src_index"])
    return [dict(xy=xy[b, :n], idp=idp[b, :n], src=src[b, :n]) for b, n in enumerate(r["n"])]


def _same_maps(a, b):
    return len(a) == len(b) and all(same(x[k], y[k]) for x, y in zip(a, b) for k in ("xy", "idp", "src"))


def test_depth_maps_equal_host_restatement_and_oracle(cases, refs):
    for c in cases:
        w = open_window(c)
        ref = refs[c["name"]]["maps"]
        assert _same_maps(mh.window_depth_maps(*win_args(c), c["T_dst_w"], c["K_dst"], c["dst_H"], c["dst_W"]), ref), c["name"]
        got = _maps(w, c, False)
        assert _same_maps(got, ref), c["name"]
        assert _same_maps(_maps(w, c, "array"), ref), c["name"]
        assert _same_maps(_maps(w, c, "array", stride=len(c["host"]) + 5), ref), c["name"]       # a stride beyond the point count
        assert _same_maps(_maps(w, c, False), got), c["name"]                                    # a run repeats exactly
        if not c["degenerate"]:
            nsel = mc.selected(c)
            assert all(0 < len(m["idp"]) < nsel for m in got), c["name"]
        w.close()


def test_a_batch_of_maps_equals_its_singles(cases):
    for c in cases:
        if len(c["T_dst_w"]) < 2:
            continue
        w = open_window(c)
        batch = _maps(w, c, "array")
        for b in range(len(batch)):
            assert _same_maps(_maps(w, c, "array", slice(b, b + 1)), batch[b:b + 1]), (c["name"], b)
        w.close()
    assert sorted({len(c["T_dst_w"]) for c in cases})[:3] == [1, 2, 3] and max(len(c["T_dst_w"]) for c in cases) == 5


def test_inlier_edges_on_the_device():
    c, expect = mc.edge_case()
    w = open_window(c)
    m = _maps(w, c, "array")
    for b, e in enumerate(expect):
        for i, kept in e.items():
            assert (i in m[b]["src"]) == kept, (b, i)
    py = m[2]["xy"][list(m[2]["src"]).index(7)][1]
    assert py == 0.0 and np.signbit(py)                                                           # exactly -0.0 is kept
    w.close()


# -- 3. the immature cloud -----------------------------------------------------------------------------------------------------------------------

def open_immature(c, H=mc.WIN_H, W=mc.WIN_W):
    """an eds_imm holding case c: points created from pixels (the library decides which are alive), then the case's trace results"""
    F = len(c["per_host"])
    h = immature.ImmaturePoints(H, W, F, max(1, max(c["per_host"])), 1)
    h.set_host_images(0, np.stack([kc.image(300 + f, H, W) * 255.0 for f in range(F)]))
    first = np.concatenate([[0], np.cumsum(c["per_host"])])
    alive = np.zeros(first[-1], np.int32)
    for f in range(F):
        s = slice(first[f], first[f + 1])
        if c["per_host"][f]:
            alive[s] = h.create_points(f, c["uv"][s])
            mp.set_immature_trace(h, f, c["idepth_min"][s], c["idepth_max"][s], c["status"][s])
    return h, alive


def test_immature_cloud_equals_host_restatement_and_oracle(gpu):
    for c in mc.immature_cases(mh.chunk()):
        h, alive = open_immature(c)
        assert np.array_equal(alive, mc.pattern_alive(c["uv"], mc.WIN_H, mc.WIN_W)), c["name"]
        for single in (True, False):
            args = (c["per_host"], c["uv"].astype(np.float32), c["idepth_min"], c["idepth_max"], c["status"], alive, c["T_w_c"], c["calib"], c["mask"], single)
            ref, host_form = mo.immature_cloud(*args), mh.immature_cloud(*args)
            got = mp.immature_cloud(h, c["T_w_c"], c["calib"], c["mask"], single)
            assert got["n"] == len(ref["points"]) and all(same(got[k], ref[k]) and same(got[k], host_form[k]) for k in ("points", "colors", "status")), (c["name"], single)
            dev = mp.immature_cloud(h, c["T_w_c"], c["calib"], c["mask"], single, device="array")
            assert dev["n"] == got["n"] and all(same(dev[k].numpy()[:got["n"]], ref[k]) for k in ("points", "colors", "status")), (c["name"], single)
            if c["mask"]:
                assert 0 < got["n"] < sum(c["per_host"]) * (1 if single else 8) and set(got["status"].tolist()) == set(range(6))
        h.close()


def test_a_cap_one_too_small_returns_the_count_and_touches_nothing(gpu):
    c = mc.immature_cases(mh.chunk())[0]
    h, _ = open_immature(c)
    full = mp.immature_cloud(h, c["T_w_c"], c["calib"], c["mask"], False)
    n = full["n"]
    assert n > 8
    for device in (False, "array"):
        with pytest.raises(capi.EdsError) as e:
            mp.immature_cloud(h, c["T_w_c"], c["calib"], c["mask"], False, cap=n - 1, device=device)
        assert e.value.code == INV and e.value.needed == n
    # ... and through the C ABI with sentinels in the outputs: host memory, then device memory
    L, T, cal = mp._lib(), np.ascontiguousarray(c["T_w_c"]), np.ascontiguousarray(c["calib"], np.float32)
    pts, col, st, cnt = np.full((n - 1, 3), 7.0), np.full((n - 1, 4), 7.0), np.full(n - 1, 7, np.uint8), C.c_int32(-5)
    assert L.eds_map_immature_cloud(h._h, len(T), c["mask"], capi.vp(T), capi.vp(cal), 0, n - 1, capi.vp(pts), capi.vp(col), capi.vp(st), 0,
                                    C.cast(C.byref(cnt), C.c_void_p)) == INV
    assert cnt.value == n and (pts == 7.0).all() and (col == 7.0).all() and (st == 7).all()
    dp, dc, ds = (capi.DeviceArray.from_numpy(a) for a in (pts, col, st))
    assert L.eds_map_immature_cloud(h._h, len(T), c["mask"], capi.vp(T), capi.vp(cal), 0, n - 1, C.c_void_p(dp.ptr), C.c_void_p(dc.ptr), C.c_void_p(ds.ptr), 1,
                                    C.cast(C.byref(cnt), C.c_void_p)) == INV
    assert cnt.value == n and (dp.numpy() == 7.0).all() and (dc.numpy() == 7.0).all() and (ds.numpy() == 7).all()
    exact = mp.immature_cloud(h, c["T_w_c"], c["calib"], c["mask"], False, cap=n)                # a cap that just holds it
    assert exact["n"] == n and same(exact["points"], full["points"])
    h.close()


# -- 4. the cloud follows the tables ----------------------------------------------------------------------------------------------------------------

def _table_cloud_equals_oracle(w, sv, ed, K, F, seed):
    rows, ids = ed.rows(state=False), sv.get(system=False)["idepth_scaled"]
    rng = np.random.default_rng(seed)
    T = np.stack([mc.random_pose(rng) for _ in range(F)])
    calib = np.array(K, np.float32)
    for single in (True, False):
        ref, per_ref = mo.window_cloud(rows["host"], rows["uv"], ids, calib, T, (1 << F) - 1, single)
        got, per = mp.window_cloud(w, T, None, single)
        assert len(ref) == w.n * (1 if single else 8) and same(got, ref) and np.array_equal(per, per_ref)
    Td, Kd = mc.destinations(rng, 2, 40, 50)
    ref = mo.window_depth_maps(rows["host"], rows["uv"], ids, calib, T, (1 << F) - 1, Td, Kd, 40, 50)
    r = mp.window_depth_maps(w, T, Td, Kd, 40, 50)
    assert all(same(r["depth_idp"][b, :r["n"][b]], ref[b]["idp"]) and same(r["src_index"][b, :r["n"][b]], ref[b]["src"]) for b in range(2))
    return ids


def test_the_cloud_follows_a_step_and_a_removal(gpu):
    s = wec.cases()["f3_513"]
    c = s.win
    w, sv = wsh.open_case(s, window.Window, winsolve.WindowSolver, max_points=len(c.host), max_residuals=len(c.point))
    ed = winedit.WindowEdit(w, sv)
    weh.prepare(w, sv, s)                                        # ... -> solve -> eds_wsv_step_idepths
    ids = _table_cloud_equals_oracle(w, sv, ed, c.K, s.F, 1)
    assert not np.array_equal(ids, np.asarray(c.ids, np.float32))                # the cloud read the STEPPED depths
    flag = (np.arange(w.n) % 3 == 1).astype(np.int32)
    removed, _ = ed.remove_points(flag)
    assert removed == flag.sum() and w.n == len(flag) - removed
    after = _table_cloud_equals_oracle(w, sv, ed, c.K, s.F, 2)
    assert same(after, ids[flag == 0])
    w.close()


def _activation(c):
    """an eds_imm that holds activation case c, traced as its oracle traced it, with the map, the selection and the fit made"""
    act = importlib.import_module("slam-eds_amd.activate")
    h = immature.ImmaturePoints(c.H, c.W, c.F, max(1, max(len(x["uv"]) for x in c.hosts)), 4)
    h.set_host_images(0, np.stack(c.images))
    h.set_target_images(0, np.stack(c.trace_targets))
    for i, x in enumerate(c.hosts):
        h.create_points(i, x["uv"], x["type"])
    for k, step in enumerate(c.trace_steps):
        h.trace(0, [k] * c.F, np.stack([s[0] for s in step]), np.stack([s[1] for s in step]), np.stack([s[2] for s in step]))
    a = act.Activation(h, *c.K4, **c.act_prm)
    a.make_distance_map(c.newest, c.KRKi1, c.Kt1, c.active_host, c.active)
    a.select(c.newest, c.KRKi1, c.Kt1, c.flagged, c.min_dist)
    a.optimize(c.pre)
    return h, a


def test_the_cloud_follows_an_insert_of_activated_points(gpu):
    s = wec.insert_case("w64_f3")
    c = s.win
    h, a = _activation(s.act)
    K = len(a.activated()["host"])
    assert K > 0
    w, sv = wsh.open_case(s, window.Window, winsolve.WindowSolver, max_points=len(c.host) + K, max_residuals=len(c.point) + 8 * K)
    ed = winedit.WindowEdit(w, sv)
    wec.prepare_insert(w, sv, s)
    n0 = w.n
    _table_cloud_equals_oracle(w, sv, ed, c.K, s.F, 3)
    assert ed.insert_activated(a)[0] == K and w.n == n0 + K
    _table_cloud_equals_oracle(w, sv, ed, c.K, s.F, 4)
    w.close()
    h.close()


# -- 5. the hand-over to the tracker ----------------------------------------------------------------------------------------------------------------

def _cfg():
    return capi.default_config(solver=capi.SOLVER_LM6, exec=capi.EXEC_DEVICE, max_num_iterations=4)


def test_depth_maps_go_to_the_tracker_without_leaving_the_device(gpu):
    H, W, count = 61, 83, 2
    rng = np.random.default_rng(77)
    per = [150, 0, 170, 130]
    n = sum(per)
    # a window whose field of view covers the new keyframes' and more, under real-valued poses: the maps are unambiguous for the device k-d build
    c = dict(host=np.repeat(np.arange(4), per).astype(np.int32), ids=rng.uniform(0.4, 1.6, n).astype(np.float32),
             uv=np.stack([rng.uniform(2, 92, n), rng.uniform(2, 68, n)], axis=1).astype(np.float32), calib=np.array([70.2, 69.1, 47.3, 35.4], np.float32),
             T_w_c=np.stack([mc.random_pose(rng, 0.05, 0.1) for _ in range(4)]), mask=0b1111)
    T_dst_w = np.stack([mc.inverse(mc.random_pose(rng, 0.06, 0.1)) for _ in range(count)])
    Ks = np.array([[66.0, 65.0, 41.2, 30.4], [64.5, 66.5, 40.1, 31.3]])
    ref = mo.window_depth_maps(*win_args(c), T_dst_w, Ks, H, W)
    assert all(50 < len(m["idp"]) < n for m in ref) and max(len(m["idp"]) for m in ref) <= kc.CAPACITY
    w = open_window(c, 72, 96)
    imgs = np.stack([kc.image(80 + b, H, W) for b in range(count)])
    h, g = capi.Handle(_cfg(), count, 4096, H, W), capi.Handle(_cfg(), count, 4096, H, W)
    outs, maps = mp.build_keyframes_from_window(h, capi.DeviceArray.from_numpy(imgs), Ks, w, c["T_w_c"], T_dst_w)
    assert capi.is_device_array(maps["depth_xy"]) and maps["n"].tolist() == [len(m["idp"]) for m in ref]
    want = g.build_keyframes(imgs, Ks, depth=[m["xy"] for m in ref], depth_idp=[m["idp"] for m in ref])
    for b in range(count):
        assert outs[b]["status"] == want[b]["status"] == capi.EDS_OK and outs[b]["n"] == want[b]["n"] > 0
        assert outs[b]["tree_on_host"] == want[b]["tree_on_host"]
        assert all(same(outs[b][k], want[b][k]) for k in ("coord", "idp", "weights")), b
    assert not outs[0]["tree_on_host"]                            # the device built the k-d tree of a map that never left it
    h.close(); g.close(); w.close()


# -- 6. a slot's cloud ------------------------------------------------------------------------------------------------------------------------------

def test_slot_cloud_seeded_unseeded_and_a_sub_range(gpu, synth):
    H, W = 60, 80
    als = [synth.make_alignment(500 + b, H=H, W=W, N=n) for b, n in enumerate((257, 64, 300))]
    h = capi.Handle(_cfg(), 4, 300, H, W)
    for b, al in enumerate(als):
        h.set_alignment(b, al)
    h.depth_init(1, 1, capi.DEPTH_INIT_HOST, idp=[np.asarray(als[1].idp)])                     # slot 1 is seeded, 0 and 2 are not
    rng = np.random.default_rng(5)
    T = np.stack([mc.random_pose(rng) for _ in range(3)])
    f32 = np.float32

    def want(b):
        nc = als[b].norm_coord.astype(f32)
        idp = h.depth_get(1)[0][:, 0] if b == 1 else als[b].idp.astype(f32).astype(np.float64)
        ref = mo.slot_cloud(nc[:, 0], nc[:, 1], idp, T[b])
        assert same(mh.slot_cloud(nc[:, 0], nc[:, 1], idp, T[b]), ref)
        return ref
    pts, n = mp.slot_cloud(h, T)
    assert n.tolist() == [257, 64, 300] and all(same(pts[b, :n[b]], want(b)) for b in range(3))
    dev, nd = mp.slot_cloud(h, T[1:], first=1, stride=310, device="array")                       # slots 1 and 2 only
    assert nd.tolist() == [64, 300] and all(same(dev.numpy()[b, :nd[b]], want(1 + b)) for b in range(2))
    again, _ = mp.slot_cloud(h, T)
    assert again.tobytes() == pts.tobytes()
    # refused: a slot without a keyframe, a stride below the largest N, a pose that is not finite, a batch in flight
    sentinel = np.full((1, 300, 3), 7.0)
    L, cnt = mp._lib(), np.full(1, -5, np.int32)
    raw = lambda first, T1, stride: L.eds_map_slot_cloud(h._h, first, 1, capi.vp(np.ascontiguousarray(T1)), stride, capi.vp(sentinel), 0, capi.vp(cnt))   # noqa: E731
    bad = T[0].copy()
    bad[3] = np.inf
    assert raw(3, T[0], 300) == ST and raw(0, T[0], 256) == INV and raw(0, bad, 300) == INV and raw(4, T[0], 300) == INV
    h.optimize_batch(0, 0, 1, sync=False)
    assert raw(0, T[0], 300) == ST
    h.sync()
    assert (sentinel == 7.0).all() and cnt[0] == -5
    assert raw(0, T[0], 300) == capi.EDS_OK and cnt[0] == 257 and same(sentinel[0, :257], want(0))
    h.close()


# -- 7. refused calls -----------------------------------------------------------------------------------------------------------------------------

def test_refused_window_calls_touch_nothing(cases):
    c = [x for x in cases if x["name"] == "n65"][0]
    n, F = len(c["host"]), len(c["T_w_c"])
    L = mp._lib()
    T, Td, Kd = np.ascontiguousarray(c["T_w_c"]), np.ascontiguousarray(c["T_dst_w"]), np.ascontiguousarray(c["K_dst"])
    pts, xy, idp, src = np.full((n, 3), 7.0), np.full((2, n, 2), 7.0), np.full((2, n), 7.0), np.full((2, n), 7, np.int32)
    d_pts, d_xy, d_idp, d_src = (capi.DeviceArray.from_numpy(a) for a in (pts, xy, idp, src))
    cnt, cnt2 = np.full(1, -5, np.int32), np.full(2, -5, np.int32)

    def cloud(w, F_=F, T_=T, single=1, out=pts, on_device=0):
        p = C.c_void_p(out.ptr) if isinstance(out, capi.DeviceArray) else capi.vp(out)
        return L.eds_map_window_cloud(w._h if w else None, F_, c["mask"], capi.vp(T_), single, p, on_device, capi.vp(cnt), None)

    def maps(w, F_=F, T_=T, Td_=Td, Kd_=Kd, H_=c["dst_H"], W_=c["dst_W"], stride=n, outs=(xy, idp, src), on_device=0, count=2):
        p = [C.c_void_p(o.ptr) if isinstance(o, capi.DeviceArray) else capi.vp(o) for o in outs]
        return L.eds_map_window_depth_maps(w._h if w else None, F_, c["mask"], capi.vp(T_), count, capi.vp(Td_), capi.vp(Kd_), H_, W_, stride, p[0], p[1], p[2],
                                           on_device, capi.vp(cnt2))
    bare = open_window(c, calib=False)
    assert cloud(bare) == ST and maps(bare) == ST                                # before eds_win_set_calib
    bare.close()
    w = open_window(c)

    def poisoned(a, i, v):
        b = a.copy()
        b.reshape(-1)[i] = v
        return b
    assert cloud(None) == INV and maps(None) == INV
    for bad_F in (0, 9, 7):                                                       # 7: the table holds points of host 7
        assert cloud(w, F_=bad_F) == INV and maps(w, F_=bad_F) == INV, bad_F
    assert cloud(w, T_=poisoned(T, 17, np.nan)) == INV and maps(w, T_=poisoned(T, 30, np.inf)) == INV
    assert maps(w, Td_=poisoned(Td, 13, np.nan)) == INV and maps(w, Kd_=poisoned(Kd, 6, np.inf)) == INV
    assert maps(w, Kd_=poisoned(Kd, 0, 0.0)) == INV and maps(w, Kd_=poisoned(Kd, 5, 0.0)) == INV        # a zero focal length
    assert maps(w, stride=n - 1) == INV and maps(w, count=0) == INV and maps(w, H_=0) == INV and maps(w, W_=0) == INV
    assert cloud(w, single=2) == INV and cloud(w, on_device=2) == INV and maps(w, on_device=-1) == INV
    assert cloud(w, on_device=1) == INV and maps(w, on_device=1) == INV          # host pointers called device memory: a code, not a fault
    assert maps(w, outs=(d_xy, idp, d_src), on_device=1) == INV
    small = capi.DeviceArray((n - 1, 3), np.float64)
    assert cloud(w, out=small, on_device=1) == INV                                # device memory that is too short
    assert capi.last_error()
    assert (pts == 7.0).all() and (xy == 7.0).all() and (idp == 7.0).all() and (src == 7).all() and cnt[0] == -5 and (cnt2 == -5).all()
    assert (d_xy.numpy() == 7.0).all() and (d_src.numpy() == 7).all()
    # ... and the same buffers take the results once the call is good
    assert cloud(w, out=d_pts, on_device=1) == capi.EDS_OK and cnt[0] == n and maps(w, outs=(d_xy, d_idp, d_src), on_device=1) == capi.EDS_OK
    ref = mo.window_depth_maps(*win_args(c), c["T_dst_w"], c["K_dst"], c["dst_H"], c["dst_W"])
    assert same(d_pts.numpy(), mo.window_cloud(*win_args(c), True)[0]) and cnt2.tolist() == [len(m["idp"]) for m in ref]
    assert all(same(d_idp.numpy()[b, :cnt2[b]], ref[b]["idp"]) for b in range(2))
    w.close()


def test_refused_immature_calls(gpu):
    c = mc.immature_cases(mh.chunk())[0]
    h, _ = open_immature(c)
    T = c["T_w_c"]
    assert code(mp.immature_cloud, h, T[:0], c["calib"]) == INV                  # n_hosts 0
    assert code(mp.immature_cloud, h, np.concatenate([T, T]), c["calib"]) == INV  # more than the handle's hosts
    bad = T.copy()
    bad[1, 3] = np.nan
    assert code(mp.immature_cloud, h, bad, c["calib"]) == INV
    assert code(mp.immature_cloud, h, T, [0.0, 1, 1, 1]) == INV and code(mp.immature_cloud, h, T, [1, np.inf, 1, 1]) == INV
    L, cnt, pts = mp._lib(), C.c_int32(-5), np.full((400, 3), 7.0)
    cal = np.ascontiguousarray(c["calib"], np.float32)
    assert L.eds_map_immature_cloud(h._h, len(T), c["mask"], capi.vp(np.ascontiguousarray(T)), capi.vp(cal), 1, 400, capi.vp(pts), None, None, 1,
                                    C.cast(C.byref(cnt), C.c_void_p)) == INV     # a host pointer called device memory
    assert cnt.value == -5 and (pts == 7.0).all()
    h.close()


def test_torch_tensors_when_torch_came_first(cases):
    """device=True returns torch tensors on the handle's device — where torch was imported before the library, the only order in which
    PyTorch-ROCm works (capi.torch_loaded_first); otherwise the call says so instead of failing later"""
    c = [x for x in cases if x["name"] == "n65"][0]
    w = open_window(c)
    if capi.torch_loaded_first:
        got, _ = mp.window_cloud(w, c["T_w_c"], c["mask"], True, device=True)
        assert got.is_cuda and same(got.cpu().numpy(), mo.window_cloud(*win_args(c), True)[0])
    else:
        with pytest.raises(RuntimeError):
            mp.window_cloud(w, c["T_w_c"], c["mask"], True, device=True)
    w.close()
