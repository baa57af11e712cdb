"""include/eds_hip_winedit.h on the device against csrc/eds_winedit.hpp under g++ (tests/winedit_harness.py): on f3_5, f3_513, f8_1100 and
f8_4500 (4 510 points and about 20 000 residuals: several workgroups of the scan and of the gathers) the two agree bit for bit on every
row a caller can read and on every count after every step of every flag pattern of tests/winedit_cases.py, and on what the window
does next (linearize, apply, a solve with the point steps); flags given in device memory give the same; a run equals its repetition;
a refused call changes nothing; a window that never saw an eds_wed_* call is what the suites of the other two headers pin.
eds_wed_marginalize_frame and eds_wed_set_state: frame 0, a middle frame and the last on the same windows, HM' and bM' bit for bit the
host restatement's, the tables, the image planes and the next solve as well; and one keyframe cycle on the device only."""
import functools
import importlib

import numpy as np
import pytest

import winedit_cases as wec
import winedit_harness as weh
import winsolve_harness as wsh

pytestmark = pytest.mark.gpu
capi = importlib.import_module("slam-eds_amd.capi")
window = importlib.import_module("slam-eds_amd.window")
winsolve = importlib.import_module("slam-eds_amd.winsolve")
winedit = importlib.import_module("slam-eds_amd.winedit")
NAMES = ["f3_5", "f3_513", "f8_1100", wec.BIG]


def _diff(a, b):
    fa, fb = dict(wsh.flatten(a)), dict(wsh.flatten(b))
    assert fa.keys() == fb.keys(), sorted(set(fa) ^ set(fb))
    return [k for k in fa if not wsh.same_bits(fa[k], fb[k])]


def _open_device(s, spare=0):
    c = s.win
    w, sv = wsh.open_case(s, window.Window, winsolve.WindowSolver, max_points=max(len(c.host), 1) + spare, max_residuals=max(len(c.point), 1) + spare)
    return w, sv, winedit.WindowEdit(w, sv)


def _run(s, pattern, opened, steps_of=wec.steps):
    w, sv, ed = opened
    snaps, HM, bM = weh.run_pattern(w, sv, ed, s, pattern, steps_of)
    after = weh.after_edit(w, sv, s, HM, bM, full=True, accumulate=False)
    w.close()
    return dict(snaps=snaps, HM=HM, bM=bM, after=after)


@functools.lru_cache(maxsize=None)
def _host(name, pattern):
    s = wec.cases()[name]
    w, sv = wsh.open_case(s)
    out = _run(s, pattern, (w, sv, weh.HostEdit(w)))
    sv.close()
    return out


@functools.lru_cache(maxsize=None)
def _device(name, pattern):
    return _run(wec.cases()[name], pattern, _open_device(wec.cases()[name]))


def _device_flags(pattern, s, n, m, host, point):
    """the same steps with the flags in device memory"""
    return [(kind, None if f is None else capi.DeviceArray.from_numpy(f)) for kind, f in wec.steps(pattern, s, n, m, host, point)]


@pytest.mark.parametrize("pattern", wec.PATTERNS)
@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_host_restatement_bit_for_bit(name, pattern):
    host, dev = _host(name, pattern), _device(name, pattern)
    bad = _diff(host, dev)
    assert not bad, bad[:12]
    assert np.isfinite(dev["after"]["solve"]["x"]).all()


def test_the_large_window_spans_several_workgroups():
    snaps = _host(wec.BIG, "random30")["snaps"]
    n, m = snaps[0]["counts"]
    assert n > 4 * 1024 and m > 16 * 1024 and 4000 < n < 5000 and 18000 < m < 22000
    for pattern in ("first_last", "empty_run", "host0", "host_last"):
        assert len(_host(wec.BIG, pattern)["snaps"]) >= 2


@pytest.mark.parametrize("name,pattern", [("f8_1100", "random30"), (wec.BIG, "empty_run"), (wec.BIG, "marginalised")])
def test_flags_in_device_memory_and_a_repetition_give_the_same(name, pattern):
    s = wec.cases()[name]
    again = _run(s, pattern, _open_device(s), _device_flags)
    assert not _diff(_device(name, pattern), again)


def test_a_refused_call_changes_nothing():
    s = wec.cases()["f3_513"]
    w, sv, ed = _open_device(s)
    weh.prepare(w, sv, s)
    before = weh.snapshot(w, sv, ed)
    L = winedit._lib()
    host_flags = np.ones(max(w.n, w.m), np.int32)                # pageable host memory passed as device memory
    small = capi.DeviceArray.from_numpy(np.ones(3, np.int32))    # a device range that ends before n or m words
    p, q = host_flags.ctypes.data, small.ptr
    refusals = [
        lambda: L.eds_wed_remove_points(w._h, None, 0, None, None),
        lambda: L.eds_wed_remove_points(w._h, p, 2, None, None),
        lambda: L.eds_wed_remove_residuals(w._h, p, -1, None),
        lambda: L.eds_wed_remove_points(w._h, p, 1, None, None),
        lambda: L.eds_wed_remove_residuals(w._h, p, 1, None),
        lambda: L.eds_wed_remove_points(w._h, q, 1, None, None),
        lambda: L.eds_wed_remove_residuals(w._h, q, 1, None),
        lambda: L.eds_wed_get(w._h, None),
    ]
    for call in refusals:
        assert call() == capi.ERR_INVALID
        assert (w.n, w.m) == tuple(before["counts"]) and not _diff(before, weh.snapshot(w, sv, ed))
    with pytest.raises(ValueError):
        ed.remove_points(capi.DeviceArray.from_numpy(np.zeros(w.n, np.float32)))
    assert not _diff(before, weh.snapshot(w, sv, ed))
    # before any eds_wsv state there is no backup to read; the other rows are there, and an edit works
    w2, _, ed2 = _open_device(s)
    with pytest.raises(capi.EdsError) as e:
        ed2.rows()
    assert e.value.code == capi.ERR_STATE
    rows = ed2.rows(state=False)
    assert wsh.same_bits(rows["host"], s.win.host) and wsh.same_bits(rows["point"], s.win.point) and wsh.same_bits(rows["uv"], s.win.uv)
    flag = (np.arange(w2.n) % 2).astype(np.int32)
    rp, rr = ed2.remove_points(flag)
    rows = ed2.rows(state=False)
    assert rp == flag.sum() and wsh.same_bits(rows["uv"], s.win.uv[flag == 0]) and rr == len(s.win.point) - len(rows["point"])
    assert ed2.counts()[:2] == (w2.n, w2.m) == (len(flag) - rp, len(rows["point"]))
    w2.close()
    w.close()


def test_an_edited_window_can_be_set_again_and_a_state_set_after_an_edit_is_moved():
    """eds_win_set_points after an edit fills the tables the edit left as the window's own; an eds_wsv state that is first set AFTER
    the first edit gets its second set of rows at the next edit"""
    s = wec.cases()["f3_513"]
    c = s.win
    w, sv, ed = _open_device(s)
    ed.remove_points(np.zeros(w.n, np.int32))                    # the first edit: no eds_wsv state exists yet
    hw, hsv = wsh.open_case(s)
    hed = weh.HostEdit(hw)
    for a, b, e in ((w, sv, ed), (hw, hsv, hed)):
        weh.prepare(a, b, s)
        e.remove_points(s.marg)
        e.remove_residuals(None)
    assert not _diff(weh.snapshot(hw, hsv, hed), weh.snapshot(w, sv, ed))
    w.set_points(c.host, c.uv, c.color, c.weights, c.ids, c.idz)
    w.set_residuals(c.point, c.target, c.state, c.energy)
    hw.set_points(c.host, c.uv, c.color, c.weights, c.ids, c.idz)
    hw.set_residuals(c.point, c.target, c.state, c.energy)
    for a, b in ((w, sv), (hw, hsv)):
        weh.prepare(a, b, s)
    assert not _diff(weh.snapshot(hw, hsv, hed), weh.snapshot(w, sv, ed))
    hsv.close()
    hw.close()
    w.close()


FRAME_CASES = [(name, f) for name in NAMES for f in wec.frames_of(wec.cases()[name].F)]


@functools.lru_cache(maxsize=None)
def _host_frame(name, frame):
    s = wec.cases()[name]
    w, sv = wsh.open_case(s)
    out = weh.run_frame(w, sv, weh.HostEdit(w), s, frame, wec.reduce_case)
    sv.close()
    w.close()
    return out


def _device_frame(name, frame):
    s = wec.cases()[name]
    w, sv, ed = _open_device(s)
    out = weh.run_frame(w, sv, ed, s, frame, wec.reduce_case)
    w.close()
    return out


@pytest.mark.parametrize("name,frame", FRAME_CASES)
def test_a_frame_leaves_on_the_device_as_in_the_host_restatement(name, frame):
    host, dev = _host_frame(name, frame), _device_frame(name, frame)
    bad = _diff(host, dev)
    assert not bad, bad[:12]
    assert (dev["HM"] == dev["HM"].T).all() and np.isfinite(dev["next"]["solve"]["x"]).all()
    if (name, frame) in ((wec.BIG, 4), ("f3_5", 1)):             # a run equals its repetition
        assert not _diff(dev, _device_frame(name, frame))


def test_a_refused_frame_marginalisation_changes_nothing():
    s = wec.cases()["f3_513"]
    w, sv, ed = _open_device(s)
    with pytest.raises(capi.EdsError) as e:                      # no state yet
        ed.marginalize_frame(1, s.prior[1], s.delta_prior[1], s.HM, s.bM)
    assert e.value.code == capi.ERR_STATE
    weh.prepare(w, sv, s)
    before = dict(weh.snapshot(w, sv, ed), frames=np.stack([w.frame(f) for f in range(s.F)]))
    bad = s.HM.copy()
    bad[2, 3] = np.nan
    refusals = [(capi.ERR_STATE, lambda: ed.marginalize_frame(0, s.prior[0], s.delta_prior[0], s.HM, s.bM)),             # frame 0 hosts points
                (capi.ERR_INVALID, lambda: ed.marginalize_frame(3, s.prior[0], s.delta_prior[0], s.HM, s.bM)),
                (capi.ERR_INVALID, lambda: ed.marginalize_frame(-1, s.prior[0], s.delta_prior[0], s.HM, s.bM)),
                (capi.ERR_INVALID, lambda: ed.marginalize_frame(1, s.prior[1], s.delta_prior[1], bad, s.bM)),
                (capi.ERR_INVALID, lambda: ed.marginalize_frame(1, s.prior[1], s.delta_prior[1] * np.inf, s.HM, s.bM))]
    ed.remove_points((ed.rows()["host"] == 1).astype(np.int32))
    before = dict(weh.snapshot(w, sv, ed), frames=np.stack([w.frame(f) for f in range(s.F)]))
    HM0 = s.HM.copy()
    HM0[12:20, :] = 0
    HM0[:, 12:20] = 0
    refusals.append((capi.ERR_NOT_USABLE, lambda: ed.marginalize_frame(1, np.zeros(8), np.zeros(8), HM0, s.bM)))        # a zero block, no prior
    refusals.append((capi.ERR_NOT_USABLE, lambda: ed.marginalize_frame(1, s.prior[1], s.delta_prior[1], np.full_like(s.HM, 1e300), s.bM)))
    for code, call in refusals:
        with pytest.raises(capi.EdsError) as e:
            call()
        assert e.value.code == code, (code, str(e.value))
        assert not _diff(before, dict(weh.snapshot(w, sv, ed), frames=np.stack([w.frame(f) for f in range(s.F)])))
    ed.marginalize_frame(1, s.prior[1], s.delta_prior[1], s.HM, s.bM)         # ... and the state is still good for the real call
    with pytest.raises(capi.EdsError) as e:
        sv.l_energy()                                            # F changed: the state is to be set again
    assert e.value.code == capi.ERR_STATE
    with pytest.raises(capi.EdsError) as e:
        w.frame(s.F - 1)                                         # the freed slot holds no image
    assert e.value.code == capi.ERR_STATE
    w.close()


def test_a_keyframe_cycle_on_the_device_only():
    """marginalize_points -> remove_points -> remove_residuals(NULL) -> marginalize_frame -> a new frame's image into the freed slot ->
    eds_wed_set_state -> linearize / solve, on both sides, with no table read back in between (the snapshots are taken at the end)"""
    s = wec.cases()["f8_1100"]
    frame = 2
    r = wec.reduce_case(s, frame)
    new_image = s.win.images[frame][::-1].copy()                 # the next keyframe's image: goes into slot F - 1
    out = []
    hw, hsv = wsh.open_case(s)
    for w, sv, ed in (_open_device(s), (hw, hsv, weh.HostEdit(hw))):
        weh.prepare(w, sv, s)
        marg = np.maximum(s.marg, ed.rows()["host"] == frame).astype(np.int32)            # the frame's points are marginalised with the others
        sv.fix_linearization(marg[ed.rows()["point"]])
        HM, bM, res_m = sv.marginalize_points(marg, s.HM, s.bM, prior_fac=wsh.PRIOR_FAC, weight_fac=wsh.WEIGHT_FAC)
        removed = [ed.remove_points(marg), ed.remove_residuals(None)]
        HM, bM = ed.marginalize_frame(frame, s.prior[frame], s.delta_prior[frame], HM, bM)
        w.set_frames(r.F, new_image)
        ed.set_state(r.F, r.win.adH, r.win.adT, r.delta, r.prior, r.delta_prior, r.cPrior, r.cDelta)
        nxt = weh.after_edit(w, sv, r, HM, bM, full=True, accumulate=False)
        out.append(dict(removed=np.array(removed[0] + (removed[1],), np.int32), res_m=np.int32(res_m), HM=HM, bM=bM, next=nxt, end=weh.snapshot(w, sv, ed),
                        frames=np.stack([w.frame(f) for f in range(s.F)])))
        w.close()
    assert not _diff(out[1], out[0])
    assert out[0]["removed"].all() and out[0]["end"]["counts"].all()


# ---- eds_wed_insert_activated -----------------------------------------------------------------------------------------------------------

def _activation(c, max_hosts=None):
    """an eds_imm that holds activation case c, traced as its oracle traced it, with the map, the selection and the fit made"""
    imm, act = importlib.import_module("slam-eds_amd.immature"), importlib.import_module("slam-eds_amd.activate")
    h = imm.ImmaturePoints(c.H, c.W, max_hosts or c.F, max(1, max(len(x["uv"]) for x in c.hosts)), 4)
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


def _lin_after(w, s):
    c = s.win
    energy, counts = w.linearize(c.F, c.precalc, c.th)
    r = w.residuals()
    J = r["J"].copy()
    J[r["new_state"] == 1] = 0
    return dict(energy=np.float64(energy), counts=counts, new_state=r["new_state"], new_energy=r["new_energy"], ret=r["linearize_return"], J=J)


@pytest.mark.parametrize("name", wec.INSERT_NAMES)
def test_activated_points_enter_on_the_device_as_in_the_host_restatement(name):
    s = wec.insert_case(name)
    h, a = _activation(s.act)
    activated = a.activated()                                    # for the host side only: the device entry point reads the eds_imm itself
    K, R = len(activated["host"]), int(sum(bin(int(x)).count("1") for x in activated["target_mask"]))
    w, sv, ed = _open_device(s, spare=K + R)
    hw, hsv = wsh.open_case(s)
    hed = weh.HostEdit(hw)
    out = []
    for ww, vv, ee, arg in ((w, sv, ed, a), (hw, hsv, hed, None)):
        wec.prepare_insert(ww, vv, s)
        got = ee.insert_activated(arg) if arg is not None else ee.insert_activated(activated, s.F)
        assert got == (K, R)
        if arg is not None:
            with pytest.raises(capi.EdsError) as e:              # the linearized mark is cleared
                ww.apply(True)
            assert e.value.code == capi.ERR_STATE
        out.append(dict(after=weh.snapshot(ww, vv, ee), next=_lin_after(ww, s)))
        ww.apply(True)
        out[-1]["applied"] = ww.residuals()
    assert not _diff(out[1], out[0])
    hsv.close()
    hw.close()
    w.close()
    h.close()


def test_a_refused_insert_changes_nothing():
    imm = importlib.import_module("slam-eds_amd.immature")
    act = importlib.import_module("slam-eds_amd.activate")
    s = wec.insert_case("w64_f3")
    c = s.act
    h, a = _activation(c)
    K = len(a.activated()["host"])
    assert K > 0
    for spare_p, spare_r in ((K - 1, 4096), (4096, 1)):          # capacity exceeded: points, then residuals
        w, sv = wsh.open_case(s, window.Window, winsolve.WindowSolver, max_points=len(s.win.host) + spare_p, max_residuals=len(s.win.point) + spare_r)
        ed = winedit.WindowEdit(w, sv)
        wec.prepare_insert(w, sv, s)
        before = weh.snapshot(w, sv, ed)
        with pytest.raises(capi.EdsError) as e:
            ed.insert_activated(a)
        assert e.value.code == capi.ERR_STATE and not _diff(before, weh.snapshot(w, sv, ed))
        w.apply(True)                                            # the linearized mark is still there
        w.close()
    w, sv, ed = _open_device(s, spare=4096)
    wec.prepare_insert(w, sv, s)
    before = weh.snapshot(w, sv, ed)
    other = imm.ImmaturePoints(c.H + 8, c.W, c.F, 16, 4)         # a mismatched eds_imm: another shape
    nofit = imm.ImmaturePoints(c.H, c.W, c.F, 16, 4)             # the right shape, no fit
    bad_shape, no_fit = act.Activation(other, *c.K4), act.Activation(nofit, *c.K4)
    h8, a8 = _activation(ac_cases()["m96_f8_obs3"])             # a fit over 8 hosts of another shape
    for code, arg in ((capi.ERR_INVALID, bad_shape), (capi.ERR_STATE, no_fit), (capi.ERR_INVALID, a8)):
        with pytest.raises(capi.EdsError) as e:
            ed.insert_activated(arg)
        assert e.value.code == code, str(e.value)
        assert not _diff(before, weh.snapshot(w, sv, ed))
    assert winedit._lib().eds_wed_insert_activated(w._h, None, None, None) == capi.ERR_INVALID
    assert winedit._lib().eds_wed_insert_activated(None, h._h, None, None) == capi.ERR_INVALID
    assert ed.insert_activated(a)[0] == K                        # ... and the real call still works
    for x in (w, other, nofit, h8, h):
        x.close()


def ac_cases():
    import activate_cases
    return activate_cases.cases()


def test_accumulate_on_an_edited_device_window():
    """eds_win_accumulate right after an edit reads the host copies and the rebuilt (point, target) map of the device entry point, which
    the g++ harness does not share: no residual is linearized here, so the host window's accumulate is comparable"""
    import copy
    s = copy.copy(wec.cases()["f8_1100"])
    s.fix = np.zeros_like(s.fix)
    out = []
    hw, hsv = wsh.open_case(s)
    for w, sv, ed in (_open_device(s), (hw, hsv, weh.HostEdit(hw))):
        snaps, HM, bM = weh.run_pattern(w, sv, ed, s, "random30", wec.steps)
        out.append(weh.after_edit(w, sv, s, HM, bM, full=True, accumulate=True))
        w.close()
    assert "accumulated" in out[0] and not _diff(out[1], out[0])


def test_a_whole_keyframe_cycle_with_an_eds_imm_on_the_device_only():
    """F = 4, 96 x 128: marginalize_points -> remove_points -> remove_residuals(NULL) -> marginalize_frame -> the new frame's image into
    the freed slot -> insert_activated from an eds_imm -> eds_wed_set_state -> linearize / solve, against the host harness driven
    through the same calls (the harness takes the activated points as eds_act_get_activated returns them).  The eds_imm is an
    activation case of its own over four frames; its hosts are the window's slots after the new image is in."""
    s = wec.cycle_case()
    c, frame = s.win, 1
    h, a = _activation(s.act)
    activated = a.activated()
    K, R = len(activated["host"]), int(sum(bin(int(x)).count("1") for x in activated["target_mask"]))
    assert K > 0 and R > 0
    r = wec.reduce_case(s, frame)
    out = []
    hw, hsv = wsh.open_case(s)
    for w, sv, ed, arg in (_open_device(s, spare=K + R) + (a,), (hw, hsv, weh.HostEdit(hw), None)):
        wec.prepare_insert(w, sv, s)
        marg = np.maximum(np.arange(w.n) % 3 == 0, ed.rows()["host"] == frame).astype(np.int32)
        sv.fix_linearization(marg[ed.rows()["point"]])
        HM, bM, res_m = sv.marginalize_points(marg, s.HM, s.bM, prior_fac=wsh.PRIOR_FAC, weight_fac=wsh.WEIGHT_FAC)
        removed = ed.remove_points(marg) + (ed.remove_residuals(None),)
        HM, bM = ed.marginalize_frame(frame, s.prior[frame], s.delta_prior[frame], HM, bM)
        w.set_frames(0, c.images)                                # the frames the eds_imm was made over: the new image in slot 3
        ins = ed.insert_activated(arg) if arg is not None else ed.insert_activated(activated, s.F)
        ed.set_state(s.F, c.adH, c.adT, s.delta, s.prior, s.delta_prior, s.cPrior, s.cDelta)
        HM4, bM4 = np.eye(s.N) * 1e3, np.zeros(s.N)
        HM4[:s.N - 8, :s.N - 8] = HM
        bM4[:s.N - 8] = bM
        nxt = weh.after_edit(w, sv, s, HM4, bM4, full=True, accumulate=False)
        out.append(dict(removed=np.array(removed, np.int32), inserted=np.array(ins, np.int32), res_m=np.int32(res_m), HM=HM, bM=bM, next=nxt,
                        end=weh.snapshot(w, sv, ed)))
        w.close()
    assert not _diff(out[1], out[0])
    assert tuple(out[0]["inserted"]) == (K, R) and out[0]["removed"][0] > 0 and len(r.delta) == 3
    h.close()
