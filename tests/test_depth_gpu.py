"""The inverse-depth filter on the device (include/eds_hip_depth.h) against the DepthPoints oracle (tests/np_depth_oracle.py), and
its contract with the tracker: filtered depths feed the next solve exactly as eds_trk_set_idepth would, batch = singles, seeds follow
getCoord's compaction, errors leave the state alone."""
import numpy as np
import pytest

import np_depth_oracle as do

pytestmark = pytest.mark.gpu

H, W = 120, 160
MIN_D, MAX_D, THR = 0.5, 6.0, 100.0
REL = 1e-9          # fp64 on both sides, no contraction on the device: what differs is OCML's vs the host's acos / sin / exp (1 ulp)


def _inverse(p, q):
    R = do.quat_to_R(q)
    return -R.T @ p, np.array([-q[0], -q[1], -q[2], q[3]])


def _pose(rng, synth, scale=0.08):
    p = rng.uniform(-scale, scale, size=3)
    q = synth.quat_from_axis_angle(rng.normal(size=3), rng.uniform(0.005, 0.03))
    return p, q


def _project(al, p, q):
    """true event-frame pixels of the keyframe points (depth 1/idp) under (p, q)"""
    X = np.column_stack([al.norm_coord, np.ones(al.N)]) / al.idp[:, None]
    Xe = X @ do.quat_to_R(q).T + p
    return np.column_stack([al.fx * Xe[:, 0] / Xe[:, 2] + al.cx, al.fy * Xe[:, 1] / Xe[:, 2] + al.cy])


def _kf_pixels(al):
    return np.column_stack([al.fx * al.norm_coord[:, 0] + al.cx, al.fy * al.norm_coord[:, 1] + al.cy])


def _rows(arrs, stride):
    t = np.zeros((len(arrs), stride, 2))
    for b, a in enumerate(arrs):
        t[b, :len(a)] = a
    return t


def _close(a, b, rel=REL):
    a, b = np.asarray(a), np.asarray(b)
    return np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)) <= rel


def _same_info(ia, ib, ref12):
    """eds_trk_info of two solves on identical inputs: equal, except that REF12's reported costs carry a last-bit run-to-run spread of
    the solver itself (the same handle solving the same slot twice reports costs 1 ulp apart; its poses are bit-stable)"""
    ia, ib = dict(ia), dict(ib)
    for k in ("time_seconds", "meas_time_us", "device_time_us") + (("initial_cost", "final_cost") if ref12 else ()):
        a, b = ia.pop(k, None), ib.pop(k, None)
        if k.endswith("cost"):
            assert a == pytest.approx(b, rel=1e-14, abs=0)
    assert ia == ib


def _setup(capi, synth, als, cfg=None):
    cfg = cfg or capi.default_config(solver=capi.SOLVER_LM6, exec=capi.EXEC_DEVICE, max_num_iterations=6)
    h = capi.Handle(cfg, len(als), max(a.N for a in als), H, W)
    for b, a in enumerate(als):
        h.set_alignment(b, a)
    return h


def _run_parity(capi, synth, als, coords, with_kf, explicit_T, steps, seed):
    rng = np.random.default_rng(seed)
    B = len(als)
    h = _setup(capi, synth, als)
    idp0 = [a.idp * (1.0 + rng.normal(scale=0.05, size=a.N)) for a in als]
    h.depth_init(0, B, capi.DEPTH_INIT_HOST, idp=idp0, min_depth=MIN_D, max_depth=MAX_D, threshold=THR)
    prms = [do.Params(do.K_matrix(a.fx, a.fy, a.cx, a.cy), MIN_D, MAX_D, THR) for a in als]
    seeds = [do.init_vector(prms[b], idp0[b]) for b in range(B)]
    stride = max(a.N for a in als)
    for step in range(steps):
        states = [_pose(rng, synth) for _ in range(B)]
        h.set_states(0, np.array([s[0] for s in states]), np.array([s[1] for s in states]), np.stack([a.v0 for a in als]))
        Ts = [_pose(rng, synth) for _ in range(B)] if explicit_T else None
        kf_true = [_kf_pixels(a) for a in als]
        kf = kf_true if with_kf else [do.slot_pixels(a.norm_coord, (a.fx, a.fy, a.cx, a.cy)) for a in als]
        xy, want = [], []
        for b, a in enumerate(als):
            p, q = states[b]
            if explicit_T:
                R, t, tke = do.T_ef_kf_from(T_kf_ef=Ts[b])
                pe, qe = _inverse(*Ts[b])
            else:
                R, t, tke = do.T_ef_kf_from(p=p, q=q)
                pe, qe = p, q
            ef = _project(a, pe, qe) + rng.normal(scale=0.3, size=(a.N, 2))
            if coords == capi.DEPTH_EF_COORD:
                xy.append(ef); ef_o = ef
            elif coords == capi.DEPTH_TRACKS:
                xy.append(ef - kf_true[b]); ef_o = kf[b] + (ef - kf_true[b])
            else:
                rho = seeds[b][:, 0].astype(np.float32)
                ef_o = kf[b] + do.reproject_tracks(a.norm_coord, rho, (a.fx, a.fy, a.cx, a.cy), p, q)
            want.append(do.update(prms[b], seeds[b], kf[b], ef_o, R, t, tke))
        T7 = np.array([np.concatenate(T) for T in Ts]) if explicit_T else None
        got = h.depth_update(0, B, coords, xy=_rows(xy, stride) if xy else None, kf_xy=_rows(kf_true, stride) if with_kf else None,
                             T_kf_ef=T7)
        assert got == want, (step, got[:3], want[:3])
    for b in range(B):
        s, conv = h.depth_get(b)
        assert _close(s, seeds[b]), (b, np.max(np.abs(s - seeds[b]) / np.abs(seeds[b])))
        th = prms[b].mu_range / THR
        assert np.array_equal(conv, seeds[b][:, 1] < th * th)
        assert np.array_equal(h.depth_get_idepth(b), s[:, 0])
    h.close()


@pytest.mark.parametrize("coords", [0, 1, 2])
@pytest.mark.parametrize("with_kf", [True, False])
@pytest.mark.parametrize("explicit_T", [True, False])
def test_parity_64_ragged(gpu, capi, synth, coords, with_kf, explicit_T):
    als = [synth.make_alignment(300 + b, H=H, W=W, N=2000 - 29 * b) for b in range(64)]
    _run_parity(capi, synth, als, coords, with_kf, explicit_T, steps=10, seed=coords * 4 + with_kf * 2 + explicit_T)


@pytest.mark.parametrize("coords", [0, 1, 2])
def test_parity_single(gpu, capi, synth, coords):
    _run_parity(capi, synth, [synth.make_alignment(41, H=H, W=W, N=2000)], coords, True, False, steps=10, seed=11)


def test_parity_4096(gpu, capi, synth):
    base = [synth.make_alignment(500 + k, H=H, W=W, N=2000) for k in range(8)]
    _run_parity(capi, synth, [base[b % 8] for b in range(4096)], capi.DEPTH_TRACKS, True, False, steps=2, seed=5)


def test_slot_pixels_against_exact_pixels(gpu, capi, synth):
    """kf_xy NULL: the keyframe pixels are an integer cell + an fp32 fraction (~6e-8 px at most off the fp64 pixel).  Against the
    oracle on the exact pixels mu may move by that much of the disparity: |dmu| / mu <= 6e-8 px * 20 / disparity."""
    rng = np.random.default_rng(3)
    al = synth.make_alignment(77, H=H, W=W, N=2000)
    h = _setup(capi, synth, [al])
    h.depth_init(0, 1, capi.DEPTH_INIT_HOST, idp=al.idp[None], min_depth=MIN_D, max_depth=MAX_D)
    p, q = np.array([0.1, -0.05, 0.02]), synth.quat_from_axis_angle([0.2, 1.0, -0.3], 0.01)
    h.set_state(0, p, q, al.v0)
    kf = _kf_pixels(al)
    ef = _project(al, p, q) + rng.normal(scale=0.3, size=(al.N, 2))
    h.depth_update(0, 1, capi.DEPTH_EF_COORD, xy=ef[None])
    prm = do.Params(do.K_matrix(al.fx, al.fy, al.cx, al.cy), MIN_D, MAX_D)
    s = do.init_vector(prm, al.idp)
    R, t, tke = do.T_ef_kf_from(p=p, q=q)
    do.update(prm, s, kf, ef, R, t, tke)
    disparity = np.linalg.norm(ef - kf, axis=1)
    got = h.depth_get(0)[0][:, 0]
    assert np.all(np.abs(got - s[:, 0]) <= np.abs(s[:, 0]) * 6e-8 * 20 / np.maximum(disparity, 1e-3) + 1e-15)
    h.close()


@pytest.mark.parametrize("solver", ["LM6", "REF12"])
def test_depth_update_then_optimize_equals_set_idepth(gpu, capi, synth, solver):
    al = synth.make_alignment(21, H=H, W=W, N=1500)
    s = capi.SOLVER_LM6 if solver == "LM6" else capi.SOLVER_REF12
    cfg = capi.default_config(solver=s, exec=capi.EXEC_DEVICE, max_num_iterations=8, num_blocks=1 if solver == "LM6" else 3)
    ha, hb = _setup(capi, synth, [al], cfg), _setup(capi, synth, [al], cfg)
    rng = np.random.default_rng(1)
    ha.depth_init(0, 1, capi.DEPTH_INIT_HOST, idp=(al.idp * (1 + rng.normal(scale=0.1, size=al.N)))[None], min_depth=MIN_D, max_depth=MAX_D)
    p, q = np.array([0.08, 0.02, -0.03]), synth.quat_from_axis_angle([1.0, 0.3, 0.2], 0.02)
    ha.set_state(0, p, q, al.v0)
    ef = _project(al, p, q) + rng.normal(scale=0.3, size=(al.N, 2))
    ha.depth_update(0, 1, capi.DEPTH_EF_COORD, xy=ef[None])
    hb.set_idepth(0, ha.depth_get_idepth(0))
    ra = ha.optimize(0, p=al.p0, q=al.q0, v=al.v0)
    rb = hb.optimize(0, p=al.p0, q=al.q0, v=al.v0)
    for x, y in zip(ra[:3], rb[:3]):
        assert np.array_equal(x, y)
    _same_info(ra[3], rb[3], solver == "REF12")
    assert np.array_equal(ha.residuals(0), hb.residuals(0))
    ha.close(); hb.close()


def test_batch_equals_singles(gpu, capi, synth):
    als = [synth.make_alignment(600 + b, H=H, W=W, N=1200 + 50 * b) for b in range(8)]
    cfg = capi.default_config(solver=capi.SOLVER_REF12, exec=capi.EXEC_DEVICE, max_num_iterations=6, num_blocks=3)
    ha, hb = _setup(capi, synth, als, cfg), _setup(capi, synth, als, cfg)
    rng = np.random.default_rng(2)
    for h in (ha, hb):
        h.depth_init(0, 8, capi.DEPTH_INIT_PLANE, min_depth=MIN_D, max_depth=MAX_D)
    states = [_pose(rng, synth) for _ in range(8)]
    P, Q, V = np.array([s[0] for s in states]), np.array([s[1] for s in states]), np.stack([a.v0 for a in als])
    ha.set_states(0, P, Q, V); hb.set_states(0, P, Q, V)
    tr = [(_project(a, *states[b]) + rng.normal(scale=0.3, size=(a.N, 2))) - _kf_pixels(a) for b, a in enumerate(als)]
    sa = ha.depth_update(0, 8, capi.DEPTH_TRACKS, xy=tr)
    sb = [hb.depth_update(b, 1, capi.DEPTH_TRACKS, xy=[tr[b]])[0] for b in range(8)]
    assert sa == sb
    for b in range(8):
        assert np.array_equal(ha.depth_get(b)[0], hb.depth_get(b)[0])
    # the solves that read the refreshed planes and Gram matrices (the pose-only model is built from the Gram matrices)
    for solver, nb in ((capi.SOLVER_LM6, 3), (capi.SOLVER_REF12, 3)):      # (same block count: set_config keeps the Gram matrices)
        c = capi.default_config(solver=solver, exec=capi.EXEC_DEVICE, max_num_iterations=6, num_blocks=nb)
        ha.set_config(c); hb.set_config(c)
        for b, a in enumerate(als):
            ra, rb = ha.optimize(b, p=a.p0, q=a.q0, v=a.v0), hb.optimize(b, p=a.p0, q=a.q0, v=a.v0)
            for x, y in zip(ra[:3], rb[:3]):
                assert np.array_equal(x, y)
            _same_info(ra[3], rb[3], solver == capi.SOLVER_REF12)
    ha.close(); hb.close()


def test_compaction_keeps_seeds_aligned(gpu, capi, synth):
    al = synth.make_alignment(61, H=H, W=W, N=900, margin=2)
    h = _setup(capi, synth, [al, al, al])
    # seeded with the depths the planes already hold (the planes, and so getCoord's outputs, stay those of an unseeded slot)
    h.depth_init(0, 1, capi.DEPTH_INIT_HOST, idp=al.idp[None], min_depth=MIN_D, max_depth=MAX_D)
    h.depth_init(2, 1, capi.DEPTH_INIT_PLANE, min_depth=MIN_D, max_depth=MAX_D)
    before0, before2 = h.depth_get(0)[0], h.depth_get(2)[0]
    ref = _setup(capi, synth, [al, al, al])          # never seeded: today's outputs
    p, q = np.array([0.06, -0.03, 0.01]), synth.quat_from_axis_angle([0.1, 1.0, 0.2], 0.05)
    for hh in (h, ref):
        for b in range(3):
            hh.set_state(b, p, q, al.v0)
    out = h.update_points(0, True)
    keep = out["kept"]
    assert 50 < al.N - len(keep) < al.N - 50
    assert np.array_equal(h.depth_get(0)[0], before0[keep])
    o_ref = ref.update_points(0, True)
    for k in ("coord", "tracks", "kept", "mean_sq_flow"):
        assert np.array_equal(out[k], o_ref[k])
    # the batched form: slot 1 unseeded (outputs as today), slot 2 seeded (seeds follow)
    ob = h.update_points_batch(1, 2, True)
    ob_ref = ref.update_points_batch(1, 2, True)
    for x, y in zip(ob, ob_ref):
        for k in ("coord", "tracks", "kept", "mean_sq_flow", "n"):
            assert np.array_equal(x[k], y[k])
    assert np.array_equal(h.depth_get(2)[0], before2[ob[1]["kept"]])
    # the compacted slot keeps filtering, its plane is the compacted mu
    s0 = h.depth_update(0, 1, capi.DEPTH_REPROJECT)[0]
    assert s0["updated"] + s0["skipped_nan"] == len(keep)
    h.close(); ref.close()


def test_convergence_and_statistics(gpu, capi, synth):
    """30 frames of 0.3 px tracks of a known scene (baselines up to 0.2, fx = 125): mu approaches the true inverse depth, the median
    sigma2 falls at every update and most seeds converge (threshold 10: sigma < mu_range / 10)."""
    al = synth.make_alignment(88, H=H, W=W, N=2000)
    h = _setup(capi, synth, [al])
    rng = np.random.default_rng(9)
    h.depth_init(0, 1, capi.DEPTH_INIT_CONSTANT, min_depth=MIN_D, max_depth=MAX_D, threshold=10.0)
    err0 = np.median(np.abs(h.depth_get_idepth(0) - al.idp))
    s2_prev, conv = np.median(h.depth_get(0)[0][:, 1]), []
    for k in range(30):
        p, q = _pose(rng, synth, 0.2)
        h.set_state(0, p, q, al.v0)
        tr = _project(al, p, q) + rng.normal(scale=0.3, size=(al.N, 2)) - _kf_pixels(al)
        conv.append(h.depth_update(0, 1, capi.DEPTH_TRACKS, xy=tr[None])[0]["converged"])
        s2 = np.median(h.depth_get(0)[0][:, 1])
        assert s2 < s2_prev
        s2_prev = s2
    mu = h.depth_get_idepth(0)
    assert np.median(np.abs(mu - al.idp)) < 0.15 * err0
    assert conv[0] == 0 and conv[-1] > al.N // 2
    st = h.depth_stats(0, 1)[0]
    m, v = do.mean_std_vector(mu)
    med, third = do.median_idepth(mu)
    assert st[0] == pytest.approx(m, rel=1e-13) and st[1] == pytest.approx(v, rel=1e-12)      # fp64 sums in another order
    assert st[2] == med and st[3] == third                                                    # order statistics: exact
    h.close()


def test_stats_batch_and_single_point(gpu, capi, synth):
    als = [synth.make_alignment(700 + b, H=H, W=W, N=n) for b, n in enumerate((1, 2, 3, 257, 1999))]
    h = _setup(capi, synth, als)
    h.depth_init(0, len(als), capi.DEPTH_INIT_HOST, idp=[a.idp for a in als], min_depth=MIN_D, max_depth=MAX_D)
    st = h.depth_stats()
    for b, a in enumerate(als):
        m, v = do.mean_std_vector(a.idp)
        assert st[b, 0] == pytest.approx(m, rel=1e-13) and st[b, 1] == pytest.approx(v, rel=1e-12, abs=0)
        assert tuple(st[b, 2:]) == do.median_idepth(a.idp)
    assert st[0, 1] == 0.0
    h.close()


def test_depthpoints_mirror(gpu, capi, synth):
    import importlib
    depth = importlib.import_module("slam-eds_amd.depth")
    al = synth.make_alignment(90, H=H, W=W, N=500)
    h = _setup(capi, synth, [al])
    K = do.K_matrix(al.fx, al.fy, al.cx, al.cy)
    dp = depth.DepthPoints(h, 0)
    dp.init(K, al.N, MIN_D, MAX_D)
    assert dp.size() == al.N and np.all(dp.getIDepth() == 1.0 / ((MAX_D - MIN_D) / 2.0))
    dp.init(K, al.idp, MIN_D, MAX_D)
    assert np.array_equal(dp.getIDepth(), al.idp)
    dp[3] = [0.25, 1e-3, 3.0, 4.0]
    assert np.array_equal(dp[3], [0.25, 1e-3, 3.0, 4.0])
    mean, var = dp.meanIDepth()
    assert mean == pytest.approx(np.mean(dp.getIDepth()), rel=1e-13)
    p, q = np.array([0.1, 0.0, 0.02]), synth.quat_from_axis_angle([0, 1, 0], 0.01)
    h.set_state(0, p, q, al.v0)
    tr = _project(al, p, q) - _kf_pixels(al)
    s = dp.update(None, _kf_pixels(al), tr)
    assert s["updated"] == al.N
    h.close()


def test_errors_leave_state_alone(gpu, capi, synth):
    als = [synth.make_alignment(800 + b, H=H, W=W, N=600) for b in range(3)]
    cfg = capi.default_config(solver=capi.SOLVER_LM6, exec=capi.EXEC_DEVICE, max_num_iterations=4)
    h = capi.Handle(cfg, 4, 600, H, W)
    for b, a in enumerate(als):
        h.set_alignment(b, a)
    with pytest.raises(capi.EdsError) as e:
        h.depth_update(0, 1)                                        # not seeded
    assert e.value.code == capi.ERR_STATE
    with pytest.raises(capi.EdsError) as e:
        h.depth_init(3, 1)                                          # no keyframe
    assert e.value.code == capi.ERR_STATE
    h.depth_init(0, 3, capi.DEPTH_INIT_PLANE)
    before = [h.depth_get(b)[0] for b in range(3)]
    xy = np.zeros((1, 600, 2))
    for kw, code in ((dict(coords=7), capi.ERR_INVALID), (dict(coords=0, filter=5), capi.ERR_INVALID),
                     (dict(coords=0), capi.ERR_INVALID)):                              # xy missing
        with pytest.raises(capi.EdsError) as e:
            h.depth_update(0, 1, **kw)
        assert e.value.code == code
    with pytest.raises(capi.EdsError) as e:
        h.depth_update(0, 1, capi.DEPTH_TRACKS, xy=np.zeros((1, 10, 2)))               # stride below N
    assert e.value.code == capi.ERR_INVALID
    with pytest.raises(capi.EdsError) as e:
        h.depth_init(0, 1, source=9)
    assert e.value.code == capi.ERR_INVALID
    with pytest.raises(capi.EdsError) as e:
        h.depth_update(2, 3, capi.DEPTH_REPROJECT)                                     # range past the handle
    assert e.value.code == capi.ERR_INVALID
    h.optimize_batch(0, 0, 3, sync=False)                                               # a batch in flight
    with pytest.raises(capi.EdsError) as e:
        h.depth_update(0, 1, capi.DEPTH_TRACKS, xy=xy)
    assert e.value.code == capi.ERR_STATE
    with pytest.raises(capi.EdsError) as e:
        h.depth_stats(0, 3)
    assert e.value.code == capi.ERR_STATE
    h.sync()
    for b in range(3):
        assert np.array_equal(h.depth_get(b)[0], before[b])
    h.set_alignment(1, als[1])                                                          # a new keyframe unseeds
    with pytest.raises(capi.EdsError) as e:
        h.depth_get(1)
    assert e.value.code == capi.ERR_STATE
    assert h.depth_update(0, 1, capi.DEPTH_REPROJECT)[0]["updated"] >= 0
    h.close()
