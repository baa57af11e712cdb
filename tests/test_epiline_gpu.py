"""The epiline tracker on the device (include/eds_hip_epiline.h) against the numpy restatement of trackPointsAlongEpiline
(tests/np_epiline_oracle.py).  The oracle is fed what the slot holds: the keyframe pixels as cell + fp32 fraction, the fp32 gradients,
the fp32 inverse-depth plane (or the fp64 seeds), the event frame as the slot stores it.

A location is judged per method with tol(r) = 2 K 2^-24 + 2^-23 (fp32 accumulation, |dC| <= gamma_K t): where the oracle's best beats
every other position by more than 2 tol the device must return it; elsewhere the oracle's score at the device's location must be within
tol of its best.  Reported scores are within tol of the oracle's."""
import numpy as np
import pytest

import np_epiline_oracle as eo
import np_klt_oracle as ko
import subpixel_cases as sc

pytestmark = pytest.mark.gpu

VEL = np.array([0.3, -0.2, 0.5, 0.02, -0.03, 0.01])
BORDERS = [(eo.BORDER_CONSTANT, 0), (eo.BORDER_CONSTANT, 255), (eo.BORDER_REPLICATE, 0), (eo.BORDER_REFLECT, 0),
           (eo.BORDER_REFLECT_101, 0)]


def _handle(capi, als, vel=VEL, solver=None, max_points=None):
    cfg = capi.default_config(solver=capi.SOLVER_LM6 if solver is None else solver, exec=capi.EXEC_DEVICE, max_num_iterations=4)
    h = capi.Handle(cfg, len(als), max(a.N for a in als) if max_points is None else max_points, als[0].H, als[0].W)
    for b, a in enumerate(als):
        h.set_alignment(b, a)
        h.set_state(b, a.p0, a.q0, vel)
    return h


def _kpix(al):
    return eo.slot_pixels(al.norm_coord, al.fx, al.fy, al.cx, al.cy)


def _idp(h, slot, al, seeded):
    return h.depth_get_idepth(slot) if seeded else np.asarray(al.idp, np.float64).astype(np.float32).astype(np.float64)


def _grad(al):
    return np.asarray(al.grad, np.float64).astype(np.float32).astype(np.float64)


def _oracle(h, slot, al, r, border=eo.BORDER_REFLECT_101, value=0, vel=VEL, seeded=False, sample=None):
    return eo.track_points_along_epiline(_kpix(al), _grad(al), _idp(h, slot, al, seeded), vel, (al.fx, al.fy, al.cx, al.cy),
                                         h.get_event_frame(slot), r, border, value, sample=sample, with_maps=True)


def _judge(dev_xy, dev_s, maps, best_xy, best_s, r, largest):
    """per point: True where the oracle's best is strict (the device must match it); asserts the rule everywhere"""
    tl = eo.tol(r)
    n, H, W = maps.shape
    strict = np.zeros(n, bool)
    for i in range(n):
        m = maps[i].astype(np.float64).ravel()
        m = np.where(np.isfinite(m), m, -np.inf if largest else np.inf)
        b = best_xy[i][1] * W + best_xy[i][0]
        sign = -1.0 if largest else 1.0
        others = np.delete(sign * m, b)
        strict[i] = others.size == 0 or others.min() - sign * m[b] > 2 * tl
        if strict[i]:
            assert tuple(dev_xy[i]) == tuple(best_xy[i]), (i, dev_xy[i], best_xy[i], largest)
        else:
            d = dev_xy[i][1] * W + dev_xy[i][0]
            assert sign * (m[d] - m[b]) <= tl, (i, m[d], m[b])
        assert abs(dev_s[i] - best_s[i]) <= tl, (i, dev_s[i], best_s[i])
    return strict


def _model_frame(h, slot, al, dx=2, dy=-1, noise=0.05, base=None, seed=0):
    """an event frame that holds the slot's model image shifted by (dx, dy), plus noise (or plus `base`): most points then have a
    strict best match, and the normed correlation has no exact ties"""
    model = h.epi_get_model(slot)
    H, W = model.shape
    f = np.zeros_like(model)
    f[max(dy, 0):H + min(dy, 0), max(dx, 0):W + min(dx, 0)] = model[max(-dy, 0):H - max(dy, 0), max(-dx, 0):W - max(dx, 0)]
    extra = np.random.default_rng(seed).normal(size=(H, W)) if base is None else np.asarray(base, np.float64)
    f = f + noise * np.abs(model).max() * extra / max(np.abs(extra).max(), 1e-300)
    h.set_event_frame(slot, f)
    h.set_state(slot, al.p0, al.q0, VEL)
    return f


def _check(out, ref, r, idx=None, min_strict=0.5, min_strict_ncc=None):
    idx = np.arange(len(out["ssd"])) if idx is None else np.asarray(idx)
    ssd, ncc, scr = out["ssd"][idx], out["ncc"][idx], out["scores"][idx]
    s1 = _judge(ssd, scr[:, 0], ref["ssd_map"], ref["ssd"], ref["s_ssd"], r, False)
    s2 = _judge(ncc, scr[:, 1], ref["ncc_map"], ref["ncc"], ref["s_ncc"], r, True)
    assert s1.mean() >= min_strict, s1.mean()
    if min_strict_ncc is not None:
        assert s2.mean() >= min_strict_ncc, s2.mean()
    same = np.all(ssd == ref["ssd"], axis=1) & np.all(ncc == ref["ncc"], axis=1)
    assert np.array_equal(eo.cull(ssd, ncc)[same], ref["keep"][same])
    return same


@pytest.mark.parametrize("H,W,N", [(120, 160, 300), (480, 640, 2000)])
@pytest.mark.parametrize("layout", ["uniform", "edges"])
@pytest.mark.parametrize("seeded", [False, True])
def test_model_image(gpu, capi, synth, H, W, N, layout, seeded):
    al = synth.make_alignment(7 + H, H=H, W=W, N=N, layout=layout)
    h = _handle(capi, [al])
    if seeded:
        h.depth_init(0, 1, capi.DEPTH_INIT_HOST, idp=[np.asarray(al.idp) * 1.1])
    got = h.epi_get_model(0)
    ref = eo.model_image(_kpix(al), _grad(al), _idp(h, 0, al, seeded), VEL, (al.fx, al.fy, al.cx, al.cy), H, W)
    assert np.abs(ref).max() > 0
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    h.close()


@pytest.mark.parametrize("dx,dy", [(3, -2), (0, 0), (-5, 4)])
def test_known_answer_shifted_model(gpu, capi, synth, dx, dy):
    r = 7
    al = synth.make_alignment(31, H=120, W=160, N=150)
    h = _handle(capi, [al])
    model = h.epi_get_model(0)
    frame = np.zeros_like(model)
    H, W = model.shape
    ys, xs = slice(max(dy, 0), H + min(dy, 0)), slice(max(dx, 0), W + min(dx, 0))
    frame[ys, xs] = model[max(-dy, 0):H - max(dy, 0), max(-dx, 0):W - max(dx, 0)]
    h.set_event_frame(0, frame)
    h.set_state(0, al.p0, al.q0, VEL)
    ref = _oracle(h, 0, al, r)
    out = h.epi_track_points(0, 1, r, erase=False)[0]
    kp = np.trunc(_kpix(al)).astype(np.int64)
    inner = (kp[:, 0] - r + dx >= 0) & (kp[:, 0] + r + dx < W) & (kp[:, 1] - r + dy >= 0) & (kp[:, 1] + r + dy < H) & \
            (kp[:, 0] - r >= 0) & (kp[:, 0] + r < W) & (kp[:, 1] - r >= 0) & (kp[:, 1] + r < H)
    assert inner.sum() > 50
    want = kp + np.array([dx, dy])
    assert np.array_equal(ref["ssd"][inner], want[inner])
    assert np.array_equal(out["ssd"][inner], want[inner])
    _check(out, ref, r)
    h.close()


@pytest.mark.parametrize("r", [0, 1, 3, 7, 11, 15])
@pytest.mark.parametrize("border,value", BORDERS)
def test_parity_small(gpu, capi, synth, r, border, value):
    al = synth.make_alignment(40 + r, H=120, W=160, N=80, layout="edges" if r % 2 else "uniform")
    h = _handle(capi, [al])
    _model_frame(h, 0, al, seed=r)
    ref = _oracle(h, 0, al, r, border, value)
    out = h.epi_track_points(0, 1, r, border, value, erase=False)[0]
    _check(out, ref, r)
    h.close()


def test_parity_vga_after_solve(gpu, capi, synth):
    r = 7
    al = synth.make_alignment(55, H=480, W=640, N=2000)
    h = _handle(capi, [al])
    p, q, v, _ = h.optimize(0, p=al.p0, q=al.q0, v=al.v0)
    h.set_state(0, p, q, v)
    # the solved state's model, shifted, over the solve's own event frame
    model = h.epi_get_model(0)
    frame = np.roll(model, (-2, 3), axis=(0, 1)) + 0.2 * np.abs(model).max() * h.get_event_frame(0) / np.abs(h.get_event_frame(0)).max()
    h.set_event_frame(0, frame)
    h.set_state(0, p, q, v)
    out = h.epi_track_points(0, 1, r)[0]
    sample = np.random.default_rng(0).choice(al.N, 128, replace=False)
    ref = _oracle(h, 0, al, r, vel=v, sample=sample)
    _check(out, ref, r, idx=sample)
    keep_dev = eo.cull(out["ssd"], out["ncc"])
    assert np.array_equal(np.flatnonzero(keep_dev), out["kept"]) and out["n"] == keep_dev.sum()
    assert np.array_equal(out["ef"], out["ssd"][out["kept"]].astype(np.float64))
    assert np.array_equal(h.epi_get(0), out["ef"])
    h.close()


def test_zero_velocity_zero_frame_and_nan_patch(gpu, capi, synth):
    al = synth.make_alignment(77, H=120, W=160, N=200)
    h = _handle(capi, [al], vel=np.zeros(6))
    out = h.epi_track_points(0, 1, 7)[0]
    assert (out["ssd"] == 0).all() and (out["ncc"] == 0).all() and out["n"] == al.N
    assert np.array_equal(out["kept"], np.arange(al.N))
    h.close()
    h = _handle(capi, [al])
    h.set_event_frame(0, np.zeros((al.H, al.W)))
    h.set_state(0, al.p0, al.q0, VEL)
    out = h.epi_track_points(0, 1, 5, erase=False)[0]
    assert (out["ssd"] == 0).all() and (out["scores"][:, 0] == 1.0).all()
    frame = np.array(al.frame, dtype=np.float64)
    frame[50:60, 70:90] = np.nan
    h.set_event_frame(0, frame)
    h.set_state(0, al.p0, al.q0, VEL)
    out = h.epi_track_points(0, 1, 3, erase=False)[0]
    ref = _oracle(h, 0, al, 3, sample=np.arange(40))
    _check(out, ref, 3, idx=np.arange(40), min_strict=0.3)
    for xy in (out["ssd"], out["ncc"]):
        near = (xy[:, 0] >= 70 - 3) & (xy[:, 0] < 90 + 3) & (xy[:, 1] >= 50 - 3) & (xy[:, 1] < 60 + 3)
        assert not near.any()
    h.close()


def test_batch_equals_singles_and_repeats(gpu, capi, synth):
    als = [synth.make_alignment(90 + k, H=120, W=160, N=150 + 7 * k, layout="edges" if k % 2 else "uniform") for k in range(8)]
    big = [als[k % 8] for k in range(64)]
    h = _handle(capi, big)
    for b in range(8, 64, 3):
        h.share_event_frame(b, b % 8)
    a = h.epi_track_points(0, 64, 5)
    hb = _handle(capi, big)
    for b in range(8, 64, 3):
        hb.share_event_frame(b, b % 8)
    b2 = hb.epi_track_points(0, 64, 5)
    for x, y in zip(a, b2):
        for k in ("ssd", "ncc", "scores", "ef", "kept"):
            assert np.array_equal(x[k], y[k])
    for b in (0, 5, 13, 63):
        hs = _handle(capi, [big[b]])
        s = hs.epi_track_points(0, 1, 5)[0]
        for k in ("ssd", "ncc", "scores", "ef", "kept"):
            assert np.array_equal(s[k], a[b][k]), (b, k)
        hs.close()
    h.close()
    hb.close()


def test_erasure_matches_cull_and_compaction(gpu, capi, synth, po):
    al = synth.make_alignment(123, H=120, W=160, N=400, layout="edges")
    h = _handle(capi, [al])
    h.depth_init(0, 1, capi.DEPTH_INIT_HOST, idp=[np.asarray(al.idp)])
    seeds0, _ = h.depth_get(0)
    h.klt_track_points(0, 1, 3)
    assert h._N[0] == al.N                                    # identity pose: nothing left the frame
    t0, f0 = h.klt_get(0)
    _model_frame(h, 0, al, noise=0.3, seed=5)
    full = h.epi_track_points(0, 1, 7, erase=False)[0]
    assert full["n"] == al.N and np.array_equal(h.epi_get(0), full["ssd"].astype(np.float64))
    out = h.epi_track_points(0, 1, 7)[0]
    keep = out["kept"]
    assert np.array_equal(keep, np.flatnonzero(eo.cull(full["ssd"], full["ncc"])))
    assert 0 < len(keep) < al.N, len(keep)
    assert h.depth_get(0)[0].tolist() == seeds0[keep].tolist()
    t1, f1 = h.klt_get(0)
    assert np.array_equal(t1, t0[keep]) and np.array_equal(f1, f0[keep])
    # the compacted slot solves as a keyframe uploaded with the kept points only
    al2 = type(al)(**{**al.__dict__, "norm_coord": al.norm_coord[keep], "grad": al.grad[keep], "idp": al.idp[keep],
                      "weights": al.weights[keep], "coord": al.coord[keep], "frame": h.get_event_frame(0)})
    h.set_config(capi.default_config(exec=capi.EXEC_HOST, solver=capi.SOLVER_REF12, num_blocks=3, max_num_iterations=6))
    h.depth_set(0, np.column_stack([al.idp[keep], np.ones((len(keep), 3))]))      # the plane back to the keyframe's depths
    pr, qr, vr, info = h.optimize(0, p=al.p0, q=al.q0, v=al.v0)
    ref12 = po.Oracle(al2, num_blocks=3, max_num_iterations=6).solve_lm(al.p0, al.q0, al.v0)
    assert info["num_points"] == len(keep) and info["num_iterations"] == ref12["num_iterations"]
    assert po.se3_distance(pr, qr, ref12["p"], ref12["q"]) <= 1e-4
    cfg6 = capi.default_config(exec=capi.EXEC_HOST, solver=capi.SOLVER_LM6, max_num_iterations=6)
    h.set_config(cfg6)
    g = capi.Handle(cfg6, 1, len(keep), al.H, al.W)
    g.set_alignment(0, al2)
    g.set_event_frame(0, h.get_event_frame(0))
    a, b = h.optimize(0, p=al.p0, q=al.q0, v=al.v0), g.optimize(0, p=al.p0, q=al.q0, v=al.v0)
    assert a[3]["num_points"] == len(keep)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    g.close()
    h.close()


def test_erase_zero_changes_nothing(gpu, capi, synth):
    al = synth.make_alignment(124, H=120, W=160, N=300)
    h, g = _handle(capi, [al]), _handle(capi, [al])
    h.epi_track_points(0, 1, 7, erase=False)
    assert h._N[0] == al.N
    a, b = h.optimize(0, p=al.p0, q=al.q0, v=al.v0), g.optimize(0, p=al.p0, q=al.q0, v=al.v0)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    assert np.array_equal(h.residuals(0), g.residuals(0))
    h.close()
    g.close()


def test_depth_hook_bit_identical_and_state(gpu, capi, synth):
    al = synth.make_alignment(130, H=120, W=160, N=300)
    T = np.array([[0.01, -0.02, 0.005, 0.0, 0.0, 0.0, 1.0]])
    hs = []
    for _ in range(2):
        h = _handle(capi, [al])
        h.depth_init(0, 1, capi.DEPTH_INIT_HOST, idp=[np.asarray(al.idp)])
        _model_frame(h, 0, al, noise=0.1)
        hs.append(h)
    with pytest.raises(capi.EdsError) as e:
        hs[0].epi_depth_update(0, 1, T)
    assert e.value.code == capi.ERR_STATE
    outs = [h.epi_track_points(0, 1, 7)[0] for h in hs]
    s0 = hs[0].epi_depth_update(0, 1, T)
    s1 = hs[1].depth_update(0, 1, capi.DEPTH_EF_COORD, xy=[outs[1]["ef"]], T_kf_ef=T)
    assert s0 == s1
    assert np.array_equal(hs[0].depth_get(0)[0], hs[1].depth_get(0)[0])
    h = hs[0]
    for spoil in (lambda: h.update_points(0, True), lambda: h.klt_track_points(0, 1, 3),
                  lambda: h.set_keyframe(0, al.norm_coord, al.grad, al.idp, al.weights, al.fx, al.fy, al.cx, al.cy)):
        h.set_state(0, al.p0, al.q0, VEL)
        h.set_keyframe(0, al.norm_coord, al.grad, al.idp, al.weights, al.fx, al.fy, al.cx, al.cy)
        _model_frame(h, 0, al, noise=0.1)
        h.depth_init(0, 1, capi.DEPTH_INIT_HOST, idp=[np.asarray(al.idp)])
        assert h.epi_track_points(0, 1, 3)[0]["n"] > 0
        h.epi_get(0)
        spoil()
        for call in (lambda: h.epi_get(0), lambda: h.epi_depth_update(0, 1, T)):
            with pytest.raises(capi.EdsError) as e:
                call()
            assert e.value.code == capi.ERR_STATE
    for x in hs:
        x.close()


def test_errors_leave_state_alone(gpu, capi, synth):
    al = synth.make_alignment(140, H=120, W=160, N=200)
    h = _handle(capi, [al])
    first = h.epi_track_points(0, 1, 4, erase=False)[0]
    for args in ((0, 1, 16), (0, 1, -1), (0, 1, 3, 3), (0, 1, 3, 4, 256), (0, 1, 3, 0, -1), (0, 2, 3), (1, 1, 3)):
        with pytest.raises(capi.EdsError) as e:
            h.epi_track_points(*args)
        assert e.value.code == capi.ERR_INVALID, args
    assert h._N[0] == al.N and np.array_equal(h.epi_get(0), first["ssd"].astype(np.float64))
    again = h.epi_track_points(0, 1, 4, erase=False)[0]
    assert np.array_equal(again["scores"], first["scores"])
    h2 = capi.Handle(capi.default_config(), 1, al.N, al.H, al.W)
    with pytest.raises(capi.EdsError) as e:
        h2.epi_track_points(0, 1, 3)
    assert e.value.code == capi.ERR_STATE
    h2.close()
    h.close()


def test_python_mirrors_agree_with_handle(gpu, capi, synth):
    import importlib
    trk, bat = importlib.import_module("slam-eds_amd.tracker"), importlib.import_module("slam-eds_amd.batch")
    al = synth.make_alignment(150, H=120, W=160, N=300, layout="edges")
    h = _handle(capi, [al])
    frame = _model_frame(h, 0, al, noise=0.2)
    ref = h.epi_track_points(0, 1, 7)[0]
    assert 0 < ref["n"] < al.N
    h.close()
    K = np.array([[al.fx, 0, al.cx], [0, al.fy, al.cy], [0, 0, 1.0]])
    kf = trk.KeyFrame(al.norm_coord.copy(), al.grad.copy(), al.weights.copy(), al.idp.copy(), K, al.H, al.W, coord=_kpix(al))
    t = trk.Tracker(kf, trk.Config(solver=capi.SOLVER_LM6, options=trk.SolverOptions(max_num_iterations=[4])))
    t.px, t.qx, t.vx = al.p0.copy(), al.q0.copy(), VEL.copy()
    ef = t.trackPointsAlongEpiline(frame, 7)
    assert np.array_equal(ef, ref["ef"]) and len(kf.inv_depth) == ref["n"]
    assert np.array_equal(kf.norm_coord, al.norm_coord[ref["kept"]]) and np.array_equal(kf.coord, _kpix(al)[ref["kept"]])
    t.close()
    bt = bat.BatchTracker(capi.default_config(solver=capi.SOLVER_LM6, exec=capi.EXEC_DEVICE, max_num_iterations=4), 1, al.N, al.H, al.W)
    bt.load([al])
    bt.handle.set_event_frame(0, frame)
    bt.handle.set_state(0, al.p0, al.q0, VEL)
    b = bt.track_points_along_epiline(7)[0]
    for k in ("ssd", "ncc", "scores", "ef", "kept"):
        assert np.array_equal(b[k], ref[k])
    bt.handle.close()


# -- keyframes off the pixel grid, frames that are no multiple of a tile, slot ranges that start above zero (tests/subpixel_cases.py) --

def _seed(h, capi, al, slot=0):
    h.depth_init(slot, 1, capi.DEPTH_INIT_HOST, idp=[np.asarray(al.idp) * 1.1])


def _model_parity(h, al, seeded):
    got = h.epi_get_model(0)
    kp, idp = _kpix(al), _idp(h, 0, al, seeded)
    K = (al.fx, al.fy, al.cx, al.cy)
    ref = eo.model_image(kp, _grad(al), idp, VEL, K, al.H, al.W)
    assert np.abs(ref).max() > 0
    err = np.abs(got - ref).max()
    print(f"model image {al.H}x{al.W} N={al.N} seeded={seeded}: max|got - ref| = {err:.3e}, max|ref| = {np.abs(ref).max():.3e}")
    assert err <= 1e-12 * np.abs(ref).max()
    return ko.draw_values_points(kp, eo.sparse_model(kp, _grad(al), idp, VEL, K), al.H, al.W, 0)       # the un-blurred splat


@pytest.mark.parametrize("H,W,N", [(H, W, 200) for H, W in sc.FRAMES] + [(480, 640, 2000)])
@pytest.mark.parametrize("seeded", [False, True])
def test_model_image_subpixel(gpu, capi, H, W, N, seeded):
    """all four bilinear weights at work, footprints across the seams of the 32 x 8 tiles and into their halos, partial tiles"""
    assert np.array_equal(sc.VEL, VEL)
    al = sc.subpixel_alignment(11 + H, H, W, N, extra=sc.SEAMS(H, W) + sc.LAST(H, W) + sc.EXACT)
    fr = _kpix(al) - np.floor(_kpix(al))
    assert ((fr > 0.05) & (fr < 0.95)).all(axis=1).mean() > 0.6
    h = _handle(capi, [al])
    if seeded:
        _seed(h, capi, al)
    _model_parity(h, al, seeded)
    h.close()


@pytest.mark.parametrize("H,W", sc.FRAMES)
@pytest.mark.parametrize("only", [False, True])
@pytest.mark.parametrize("seeded", [False, True])
def test_model_image_points_just_outside(gpu, capi, H, W, only, seeded):
    """keyframe pixels with x or y in (-1, 0): drawValuesPoints puts their x1 / y1 corners on column / row 0 (Utils.cpp:164-178).
    On the commit before this test the device left such points out of the image (its bins began at 0, as the KLT's, whose points
    getCoord has erased): max|got - ref| was of the order of max|ref| itself."""
    out = sc.JUST_OUTSIDE(H, W)
    al = sc.subpixel_alignment(23 + H, H, W, 0 if only else 150, extra=out if only else sc.SEAMS(H, W) + sc.LAST(H, W) + sc.EXACT + out)
    h = _handle(capi, [al])
    if seeded:
        _seed(h, capi, al)
    splat = _model_parity(h, al, seeded)
    assert np.abs(splat[0, :]).max() > 0 and np.abs(splat[:, 0]).max() > 0 and splat[0, 0] != 0      # not vacuous
    if only:
        assert not splat[1:, 1:].any()
    h.close()


@pytest.mark.parametrize("H,W,r,border,value", sc.PARITY_CASES)
def test_parity_subpixel_odd_frames(gpu, capi, H, W, r, border, value):
    al = sc.parity_alignment(H, W)
    h = _handle(capi, [al])
    _model_frame(h, 0, al, seed=r)
    ref = _oracle(h, 0, al, r, border, value)
    out = h.epi_track_points(0, 1, r, border, value, erase=False)[0]
    _check(out, ref, r, min_strict_ncc=0.5 if r >= 1 else None)
    h.close()


@pytest.mark.parametrize("N", [1, 31, 32, 33, 1023, 1024, 1025])
def test_point_count_edges(gpu, capi, N):
    """one point, the template group of 32 and the 1 024-point chunks of the ordered norm, each at and around its size, N < Np"""
    H, W, r = 37, 45, 3
    al = sc.subpixel_alignment(300 + N, H, W, N)
    h = _handle(capi, [al], max_points=1100)
    _model_parity(h, al, False)
    _model_frame(h, 0, al, seed=N)
    sample = None if N <= 33 else np.random.default_rng(N).choice(N, 64, replace=False)
    ref = _oracle(h, 0, al, r, sample=sample)
    out = h.epi_track_points(0, 1, r, erase=False)[0]
    assert len(out["ssd"]) == N and out["n"] == N
    _check(out, ref, r, idx=sample)
    h.close()


@pytest.mark.parametrize("r", [1, 3, 0])
def test_negative_best_ncc(gpu, capi, r):
    """one blob of a single sign against a frame strictly of the other sign: the best CCORR score is negative (the other branch of the
    orderable key), every SQDIFF score clamps to 1 (first index over a frame of several workgroups)"""
    H, W = 37, 45
    al = sc.subpixel_alignment(1, H, W, 0, extra=[(20.3, 15.6)])
    h = _handle(capi, [al])
    model = h.epi_get_model(0)
    assert (model >= 0).all() or (model <= 0).all()
    sign = 1.0 if model.sum() > 0 else -1.0
    h.set_event_frame(0, -sign * (1.0 + np.abs(np.random.default_rng(r).normal(size=(H, W)))))
    h.set_state(0, al.p0, al.q0, VEL)
    ref = _oracle(h, 0, al, r)
    assert ref["s_ncc"][0] < 0 and ref["s_ssd"][0] == 1.0 and tuple(ref["ssd"][0]) == (0, 0)
    out = h.epi_track_points(0, 1, r, erase=False)[0]
    print(f"r={r}: oracle ncc {ref['s_ncc'][0]:.6f} at {tuple(ref['ncc'][0])}, device {out['scores'][0, 1]:.6f} at {tuple(out['ncc'][0])}")
    _judge(out["ncc"], out["scores"][:, 1], ref["ncc_map"], ref["ncc"], ref["s_ncc"], r, True)
    assert abs(out["scores"][0, 1] - ref["s_ncc"][0]) <= eo.tol(r)
    assert tuple(out["ssd"][0]) == (0, 0) and out["scores"][0, 0] == 1.0
    if r == 0:
        assert ref["s_ncc"][0] == -1.0 and tuple(ref["ncc"][0]) == (0, 0)
        assert out["scores"][0, 1] == -1.0 and tuple(out["ncc"][0]) == (0, 0)
    else:
        assert not ref["keep"][0] and not eo.cull(out["ssd"], out["ncc"])[0]
        assert h.epi_track_points(0, 1, r)[0]["n"] == 0                           # ... and the device erases it
    h.close()


def _range_handle(capi, pairs, slots):
    """the slots `slots` of tests/subpixel_cases.range_alignments on a handle of their own: seeded, KLT planes allocated and filled"""
    als = [pairs[b][0] for b in slots]
    h = _handle(capi, als)
    for k, b in enumerate(slots):
        if pairs[b][1] != b and len(als) > 1:                                    # (on its own, a sharing slot's alignment carries its
            assert slots[k - 1] == pairs[b][1]                                    # source's frame)
            h.share_event_frame(k, k - 1)
    h.depth_init(0, len(als), capi.DEPTH_INIT_HOST, idp=[np.asarray(a.idp) for a in als])
    outs = h.klt_track_points(0, len(als), 3)
    assert [o["n"] for o in outs] == [a.N for a in als]                           # identity pose: nothing left the frame
    for k, a in enumerate(als):
        h.set_state(k, a.p0, a.q0, VEL)
    return h


def test_sub_range_equals_singles_and_leaves_the_rest(gpu, capi):
    pairs = sc.range_alignments()
    B, keys = sc.RANGE_B, ("ssd", "ncc", "scores", "ef", "kept")
    assert pairs[4][0].N >= 64 and pairs[24][0].N >= 64 and min(p[0].N for p in pairs) == 1 and max(p[0].N for p in pairs) == 300
    h, twin = _range_handle(capi, pairs, range(B)), _range_handle(capi, pairs, range(B))
    rng = np.random.default_rng(8)
    T = np.column_stack([rng.normal(scale=0.02, size=(19, 3)), np.zeros((19, 3)), np.ones(19)])

    def single(b):
        g = _range_handle(capi, pairs, [b])                                      # a sharing slot's alignment carries its source's frame
        return g, g.epi_track_points(0, 1, 5)[0]

    def same_as_single(b, out, g, s):
        for k in keys:
            assert np.array_equal(out[k], s[k]), (b, k)
        assert out["n"] == s["n"] and h._N[b] == s["n"]
        for x, y in zip(h.depth_get(b) + h.klt_get(b), g.depth_get(0) + g.klt_get(0)):
            assert np.array_equal(x, y, equal_nan=True), b
        assert np.array_equal(h.epi_get(b), s["ef"])

    outs = h.epi_track_points(5, 19, 5)                                           # one chunk of 16 and a tail of 3, starting above zero
    assert 0 < sum(o["n"] for o in outs) < sum(pairs[b][0].N for b in range(5, 24))      # the cull kept some and erased some
    singles = {}
    for b in range(5, 24):
        singles[b] = single(b)
        same_as_single(b, outs[b - 5], *singles[b])
    # (b) the slots outside the range
    for b in list(range(5)) + list(range(24, B)):
        assert h._N[b] == twin._N[b] == pairs[b][0].N
        for x, y in zip(h.depth_get(b) + h.klt_get(b), twin.depth_get(b) + twin.klt_get(b)):
            assert np.array_equal(x, y, equal_nan=True), b
        with pytest.raises(capi.EdsError) as e:
            h.epi_get(b)
        assert e.value.code == capi.ERR_STATE
    for b in (4, 24):
        al = pairs[b][0]
        x, y = h.optimize(b, p=al.p0, q=al.q0, v=al.v0), twin.optimize(b, p=al.p0, q=al.q0, v=al.v0)
        for u, w in zip(x[:3], y[:3]):
            assert np.array_equal(u, w), b
        h.set_state(b, al.p0, al.q0, VEL)
    # (c) the depth hook over the same range
    live = [b for b in range(5, 24) if outs[b - 5]["n"] > 0]
    assert len(live) == 19, "every slot of the range must keep a point for the hook to run: " + str([o["n"] for o in outs])
    summ = h.epi_depth_update(5, 19, T)
    for b in range(5, 24):
        g, s = singles[b]
        assert summ[b - 5] == g.depth_update(0, 1, capi.DEPTH_EF_COORD, xy=[s["ef"]], T_kf_ef=T[b - 5:b - 4])[0], b
        for x, y in zip(h.depth_get(b), g.depth_get(0)):
            assert np.array_equal(x, y, equal_nan=True), b
        g.close()
    # (d) a range that ends at the handle's last slot
    outs = h.epi_track_points(24, 16, 5)
    for b in range(24, B):
        g, s = single(b)
        same_as_single(b, outs[b - 24], g, s)
        g.close()
    for b in range(5):
        assert h._N[b] == pairs[b][0].N
        for x, y in zip(h.depth_get(b) + h.klt_get(b), twin.depth_get(b) + twin.klt_get(b)):
            assert np.array_equal(x, y, equal_nan=True), b
    h.close()
    twin.close()
