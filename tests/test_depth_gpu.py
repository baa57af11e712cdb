"""The inverse-depth filter on the device (include/eds_hip_depth.h) against the DepthPoints oracle (tests/np_depth_oracle.py), and
its contract with the tracker: filtered depths feed the next solve exactly as eds_trk_set_idepth would, batch = singles, seeds follow
getCoord's compaction, errors leave the state alone."""
import numpy as np
import pytest

import depth_cases as dc
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


# ---- the filter's rare branches, slot ranges, strides, 4 096+ points (tests/depth_cases.py) -------------------------------------------


def _ref12(capi, solver=None):
    return capi.default_config(solver=capi.SOLVER_REF12 if solver is None else solver, exec=capi.EXEC_DEVICE, max_num_iterations=4, num_blocks=3)


def _case_handle(capi, slots, ks, extra=0):
    """a handle whose slot b holds a keyframe of slots[b].N points with slots[b]'s intrinsics (alignment seed ks[b])"""
    als = [dc.alignment(k, s.N, K4=s.K4) for k, s in zip(ks, slots)]
    h = capi.Handle(_ref12(capi), len(slots), max(s.N for s in slots) + extra, dc.H, dc.W)
    for b, a in enumerate(als):
        h.set_alignment(b, a)
    return h, als


def _seed_case(capi, h, slots, first=0):
    h.depth_init(first, len(slots), capi.DEPTH_INIT_CONSTANT, **slots[0].params)
    for b, s in enumerate(slots):
        h.depth_set(first + b, s.seeds)


def _padded(arrs, stride, fill=0.0):
    t = np.full((len(arrs), stride) + arrs[0].shape[1:], fill)
    for b, a in enumerate(arrs):
        t[b, :len(a)] = a
    return t


def _update_case(capi, h, slots, first=0, stride=None, fill=0.0, filter=0):
    """one EDS_DEPTH_EF_COORD update of the case's slots with explicit keyframe pixels; the geometry as T_kf_ef rows or as the poses"""
    stride = stride or max(s.N for s in slots)
    T = None
    if slots[0].pose is not None:
        h.set_states(first, np.array([s.pose[0] for s in slots]), np.array([s.pose[1] for s in slots]), np.zeros((len(slots), 6)))
    else:
        T = np.array([s.T_kf_ef for s in slots])
    return h.depth_update(first, len(slots), capi.DEPTH_EF_COORD, xy=_padded([s.ef_xy for s in slots], stride, fill),
                          kf_xy=_padded([s.kf_xy for s in slots], stride, fill), T_kf_ef=T, filter=filter)


def _check_slot(h, b, slot, cls, summary, by_invariants=False):
    """seeds, flags and summary of one slot after one update against the classified oracle; returns the seeds"""
    ev, _, und = cls
    run = ev["run"]
    got, conv = h.depth_get(b)
    flags = dc.compare(slot, got, cls, restore_by_invariants=by_invariants)
    print(f"slot {b}: N {slot.N} skipped {int(flags['skipped'].sum())} restored {int(flags['restored'].sum())} reset {int(flags['reset'].sum())} "
          f"converged {int(conv.sum())}; summary {summary}")
    assert summary["updated"] == int(run.sum()) and summary["skipped_nan"] == int((~run).sum()) == int(flags["skipped"].sum())
    assert summary["mu_reset"] == int(flags["reset"].sum())
    assert summary["sigma2_restored"] == int(flags["restored"].sum())
    assert summary["converged"] == int(conv.sum())
    dec = ~und["converged"]
    assert np.array_equal(conv[dec], ev["converged"][dec])
    if not by_invariants and not (und["restore"] | und["reset"] | und["converged"]).any():
        assert summary == do.summary_of(ev)
    assert np.array_equal(h.depth_get_idepth(b), got[:, 0])
    return got


def _solves_equal_set_idepth_twin(capi, h, als, picks):
    """the LM6 and the REF12 solve of h's slots `picks` against a twin handle that got eds_trk_set_idepth(mu): bit for bit"""
    hb = capi.Handle(_ref12(capi), len(picks), h.max_points, dc.H, dc.W)
    for j, b in enumerate(picks):
        hb.set_alignment(j, als[b])
        hb.set_idepth(j, h.depth_get_idepth(b))
    for solver in (capi.SOLVER_LM6, capi.SOLVER_REF12):
        c = _ref12(capi, solver)
        h.set_config(c); hb.set_config(c)
        for j, b in enumerate(picks):
            a = als[b]
            ra, rb = h.optimize(b, p=a.p0, q=a.q0, v=a.v0), hb.optimize(j, p=a.p0, q=a.q0, v=a.v0)
            for x, y in zip(ra[:3], rb[:3]):
                assert np.array_equal(x, y, equal_nan=True), (solver, b)
            _same_info(ra[3], rb[3], solver == capi.SOLVER_REF12)
            assert np.array_equal(h.residuals(b), hb.residuals(j), equal_nan=True)
    hb.close()


def _plane_is_narrowed_mu(capi, h, first, slots, mus):
    """the slot's fp32 plane, read back through EDS_DEPTH_INIT_PLANE (mu = (double)plane): (float)mu.  This RE-SEEDS the slots: it
    must be the last thing a test does with them.  (The plane's padding, 1.0, has no reader in the API: it is pinned through the
    twin solves alone, whose kernels sweep the padded rows.)"""
    h.depth_init(first, len(slots), capi.DEPTH_INIT_PLANE, **slots[0].params)
    for b, mu in enumerate(mus):
        with np.errstate(over="ignore"):
            assert np.array_equal(h.depth_get_idepth(first + b), mu.astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("form", ["batch24", "single"])
@pytest.mark.parametrize("name", dc.CASES)
def test_branch_parity(gpu, capi, synth, name, form):
    """every case of tests/depth_cases.py as a ragged batch of 24 slots with distinct intrinsics, and slot 23 of it alone: seeds and
    flags per point and the summaries against the oracle (strictly on decided points, either outcome on the <= 1 % undecided ones;
    `cancellation` by invariants: sigma2 >= 0, sigma2 the old one bit for bit or the oracle's new one within the allowance, restored
    count = the bit-equal count >= 1, mu / a / b within tolerance whatever the branch); then plane and Gram matrices as
    eds_trk_set_idepth(mu) leaves them."""
    case = dc.make_case(name)
    ks = list(range(len(case))) if form == "batch24" else [23]
    slots = [case[k] for k in ks]
    h, als = _case_handle(capi, slots, ks)
    _seed_case(capi, h, slots)
    sums = _update_case(capi, h, slots)
    inv = name == "cancellation"
    mus, restored = [], 0
    for b, s in enumerate(slots):
        mus.append(_check_slot(h, b, s, dc.classify(s), sums[b], inv)[:, 0])
        restored += sums[b]["sigma2_restored"]
    if inv:
        assert restored >= 1
    _solves_equal_set_idepth_twin(capi, h, als, [0, 5, 23] if form == "batch24" else [0])
    _plane_is_narrowed_mu(capi, h, 0, slots, mus)
    h.close()


def _quat_pose(rng):
    return rng.uniform(-0.08, 0.08, size=3), dc.quat(rng.normal(size=3), rng.uniform(0.005, 0.03))


def _subrange_inputs(capi, rng, als, first, count, coords):
    """INIT_HOST rows, T_kf_ef rows, xy / kf_xy rows of slots first .. first + count - 1 and the oracle's result"""
    sub = als[first:first + count]
    stride = max(a.N for a in sub)
    idp0 = [a.idp * (1.0 + rng.normal(scale=0.05, size=a.N)) for a in sub]
    poses = [_quat_pose(rng) for _ in sub]
    Ts = [_quat_pose(rng) for _ in sub]
    kfs = [np.column_stack([rng.uniform(1.0, dc.W - 2.0, size=a.N), rng.uniform(1.0, dc.H - 2.0, size=a.N)]) for a in sub]
    want_seeds, want_sum, xy = [], [], []
    for j, a in enumerate(sub):
        K4 = (a.fx, a.fy, a.cx, a.cy)
        prm = do.Params(do.K_matrix(*K4), MIN_D, MAX_D, 41.0, 3.0, 4.0)
        seeds = do.init_vector(prm, idp0[j])
        R, t, tke = do.T_ef_kf_from(T_kf_ef=Ts[j])
        if coords == capi.DEPTH_REPROJECT:           # kf_xy NULL: the slot's own pixels; the track at the slot's pose from the fp32 plane
            kf = do.slot_pixels(a.norm_coord, K4)
            ef = kf + do.reproject_tracks(a.norm_coord, idp0[j].astype(np.float32), K4, *poses[j])
        else:
            kf = kfs[j]
            ef = dc.project(K4, kf, a.idp, *dc.inverse(*Ts[j])) + rng.normal(scale=0.3, size=(a.N, 2))
            xy.append(ef if coords == capi.DEPTH_EF_COORD else ef - kf)
            if coords == capi.DEPTH_TRACKS:
                ef = kf + (ef - kf)
        want_sum.append(do.update(prm, seeds, kf, ef, R, t, tke))
        want_seeds.append(seeds)
    kw = dict(T_kf_ef=np.array([np.concatenate(T) for T in Ts]))
    if coords != capi.DEPTH_REPROJECT:
        kw.update(xy=_padded(xy, stride), kf_xy=_padded(kfs, stride))
    return idp0, poses, kw, want_seeds, want_sum


@pytest.mark.parametrize("coords", [0, 1, 2])
def test_slot_subrange_against_oracle(gpu, capi, synth, coords):
    """12 ragged slots with distinct intrinsics, the calls on first = 5, count = 4: caller rows (INIT_HOST, xy, kf_xy, T_kf_ef, the
    statistics) are indexed from the range's start, planes by slot.  Against the oracle; the other eight slots keep seeds and planes
    bit for bit; the range equals four single-slot calls bit for bit."""
    first, count = 5, 4
    als = [dc.alignment(b, 640 - 31 * b, seed=coords + 1) for b in range(12)]
    prm = dict(min_depth=MIN_D, max_depth=MAX_D, threshold=41.0, init_a=3.0, init_b=4.0)
    idp0, poses, kw, want_seeds, want_sum = _subrange_inputs(capi, np.random.default_rng(40 + coords), als, first, count, coords)
    handles = []
    for _ in range(2):
        h = capi.Handle(_ref12(capi), 12, 640, dc.H, dc.W)
        for b, a in enumerate(als):
            h.set_alignment(b, a)
        h.depth_init(0, 12, capi.DEPTH_INIT_PLANE)                 # everything seeded: the range's neighbours have something to lose
        handles.append(h)
    ha, hb = handles
    outside = [b for b in range(12) if not first <= b < first + count]
    before = {b: ha.depth_get(b)[0] for b in outside}
    for h in handles:
        h.set_states(first, np.array([p for p, _ in poses]), np.array([q for _, q in poses]), np.zeros((count, 6)))
    ha.depth_init(first, count, capi.DEPTH_INIT_HOST, idp=_padded(idp0, max(len(x) for x in idp0)), **prm)
    got_sum = ha.depth_update(first, count, coords, **kw)
    print("summaries", got_sum, "oracle", want_sum)
    assert got_sum == want_sum
    st = ha.depth_stats(first, count)
    for j in range(count):
        s, conv = ha.depth_get(first + j)
        rel = np.max(np.abs(s - want_seeds[j]) / np.abs(want_seeds[j]))
        print(f"slot {first + j}: max relative seed difference {rel:.3g}")
        assert _close(s, want_seeds[j])
        th = 5.5 / 41.0
        assert np.array_equal(conv, want_seeds[j][:, 1] < th * th)
        m, v = do.mean_std_vector(s[:, 0])
        assert st[j, 0] == pytest.approx(m, rel=1e-13) and st[j, 1] == pytest.approx(v, rel=1e-12)
        assert tuple(st[j, 2:]) == do.median_idepth(s[:, 0])
    for b in outside:
        assert np.array_equal(ha.depth_get(b)[0], before[b])
    # singles
    sb = []
    for j in range(count):
        hb.depth_init(first + j, 1, capi.DEPTH_INIT_HOST, idp=idp0[j][None], **prm)
        one = {k: (v[j:j + 1] if v is not None else None) for k, v in kw.items()}
        sb.append(hb.depth_update(first + j, 1, coords, **one)[0])
    assert sb == got_sum
    for j in range(count):
        assert np.array_equal(ha.depth_get(first + j)[0], hb.depth_get(first + j)[0])
        assert np.array_equal(ha.depth_stats(first + j, 1)[0], st[j])
    # the planes of the other slots: still what set_keyframe left, (float)idp
    ha.depth_init(0, first, capi.DEPTH_INIT_PLANE); ha.depth_init(first + count, 12 - first - count, capi.DEPTH_INIT_PLANE)
    for b in outside:
        assert np.array_equal(ha.depth_get_idepth(b), als[b].idp.astype(np.float32).astype(np.float64))
    ha.close(); hb.close()


def test_stride_and_row_padding_are_never_read(gpu, capi, synth):
    """rows wider than the largest N (stride = max N + 37) and wider than the handle's Np, their padding NaN in idp, xy and kf_xy: the
    same seeds and summaries, bit for bit, as the tight rows"""
    case = dc.make_case("negative_mu_seed", n_slots=6, n0=300)
    tight = max(s.N for s in case)
    res = []
    for stride, fill in ((tight, 0.0), (tight + 37, np.nan), ((tight + 50 + 63) // 64 * 64 + 11, np.nan)):        # the last: beyond Np
        h, _ = _case_handle(capi, case, range(6), extra=50)           # Np = max N + 50, rounded up to a multiple of 64 at most
        idp = [s.seeds[:, 0] for s in case]
        h.depth_init(1, 5, capi.DEPTH_INIT_HOST, idp=_padded(idp[1:], stride, fill), min_depth=MIN_D, max_depth=MAX_D)
        h.depth_init(0, 1, capi.DEPTH_INIT_HOST, idp=_padded(idp[:1], stride, fill), min_depth=MIN_D, max_depth=MAX_D)
        init = [h.depth_get(b)[0] for b in range(6)]
        for b in range(6):
            assert np.array_equal(init[b][:, 0], idp[b]) and not np.isnan(init[b]).any()
        sums = _update_case(capi, h, case, stride=stride, fill=fill)
        res.append((sums, [h.depth_get(b)[0] for b in range(6)], h.depth_stats()))
        h.close()
    for sums, seeds, st in res[1:]:
        assert sums == res[0][0] and np.array_equal(st, res[0][2])
        for x, y in zip(seeds, res[0][1]):
            assert np.array_equal(x, y) and np.isfinite(x).all()
    assert sum(s["mu_reset"] for s in res[0][0]) > 0


def _erasing_pose():
    return np.array([0.06, -0.03, 0.01]), dc.quat([0.1, 1.0, 0.2], 0.3)


@pytest.mark.parametrize("N", [4095, 4096, 4097, 9000, 16000])
def test_compaction_beyond_one_sweep(gpu, capi, synth, N):
    """k_depth_compact gathers in sweeps of 4 096 destinations, in place: seeds after eds_trk_update_points are before[kept] bit for
    bit for N around and beyond one sweep; the compacted slot then filters against the oracle, statistics included"""
    rng = np.random.default_rng(N)
    full = dc.benign(rng, 3, N)
    full.seeds[:, 1] = rng.uniform(0.05, 1.0, size=N)
    full.seeds[:, 2:] = rng.uniform(1.0, 10.0, size=(N, 2))
    h, als = _case_handle(capi, [full], [3])
    _seed_case(capi, h, [full])
    before = h.depth_get(0)[0]
    assert np.array_equal(before, full.seeds)
    p, q = _erasing_pose()
    h.set_state(0, p, q, np.zeros(6))
    kept = h.update_points(0, True)["kept"]
    print(f"N {N}: kept {len(kept)}")
    assert 0.1 * N <= N - len(kept) <= 0.9 * N
    assert np.all(np.diff(kept) > 0)
    after = h.depth_get(0)[0]
    assert np.array_equal(after, before[kept])
    s = dc.Slot(K4=full.K4, kf_xy=full.kf_xy[kept], ef_xy=full.ef_xy[kept], seeds=after, T_kf_ef=full.T_kf_ef, special=full.special[kept])
    sums = _update_case(capi, h, [s])
    got = _check_slot(h, 0, s, dc.classify(s), sums[0])
    st = h.depth_stats(0, 1)[0]
    m, v = do.mean_std_vector(got[:, 0])
    assert st[0] == pytest.approx(m, rel=1e-13) and st[1] == pytest.approx(v, rel=1e-12)
    assert tuple(st[2:]) == do.median_idepth(got[:, 0])
    h.close()


def test_compaction_over_three_launches_of_the_batched_getcoord(gpu, capi, synth):
    """130 small ragged slots in one seeded eds_trk_update_points_batch: three launches of 64, the second and third at first + c0.
    Slots 60-63 and 70 are unseeded, every 17th slot erases everything."""
    B = 130
    rng = np.random.default_rng(130)
    ns = [40 + (7 * b) % 50 for b in range(B)]
    als = [dc.alignment(b % 24, ns[b], seed=b) for b in range(B)]
    h = capi.Handle(_ref12(capi), B, max(ns), dc.H, dc.W)
    for b, a in enumerate(als):
        h.set_alignment(b, a)
    unseeded = {60, 61, 62, 63, 70}
    for first, count in ((0, 60), (64, 6), (71, B - 71)):
        h.depth_init(first, count, capi.DEPTH_INIT_CONSTANT, min_depth=MIN_D, max_depth=MAX_D)
    before = {}
    for b in range(B):
        if b not in unseeded:
            before[b] = rng.uniform(0.1, 2.0, size=(ns[b], 4))
            h.depth_set(b, before[b])
    P = np.tile(np.array([0.06, -0.03, 0.01]), (B, 1))
    Q = np.array([dc.quat([0.1, 1.0, 0.2], 2.0 if b % 17 == 5 else 0.1 + 0.004 * b) for b in range(B)])
    h.set_states(0, P, Q, np.zeros((B, 6)))
    out = h.update_points_batch(0, B, True)
    emptied = [b for b in range(B) if out[b]["n"] == 0]
    erased = sum(ns[b] - out[b]["n"] for b in range(B))
    print("emptied slots", emptied, "erased", erased, "of", sum(ns))
    assert set(emptied) == {b for b in range(B) if b % 17 == 5} and erased > sum(ns) // 10
    partly = 0
    for b in range(B):
        o = out[b]
        if b in unseeded or o["n"] == 0:
            with pytest.raises(capi.EdsError) as e:
                h.depth_get(b)
            assert e.value.code == capi.ERR_STATE
            continue
        partly += 0 < o["n"] < ns[b]
        assert np.array_equal(h.depth_get(b)[0], before[b][o["kept"]]), b
    assert partly > B // 2
    h.close()


def _stats_want(x):
    m, v = do.mean_std_vector(x)
    xs = np.sort(x)
    return m, v, xs[len(x) // 2], xs[len(x) // 3]


def test_statistics_of_equal_keys(gpu, capi, synth):
    """EDS_DEPTH_INIT_CONSTANT, the reference's default start: every key equal, the radix select runs all eight passes.  The mean of n
    equal values is the value to n ulp (sums in another order), so the variance, exactly 0 in real numbers, may be (n ulp)^2"""
    ns = (1, 2, 3, 255, 256, 257, 2000, 16000)
    als = [dc.alignment(b, n) for b, n in enumerate(ns)]
    h = capi.Handle(_ref12(capi), len(ns), max(ns), dc.H, dc.W)
    for b, a in enumerate(als):
        h.set_alignment(b, a)
    h.depth_init(0, len(ns), capi.DEPTH_INIT_CONSTANT, min_depth=MIN_D, max_depth=MAX_D)
    mu0 = 1.0 / ((MAX_D - MIN_D) / 2.0)
    st = h.depth_stats()
    print(st)
    for b, n in enumerate(ns):
        assert np.all(h.depth_get_idepth(b) == mu0)
        assert st[b, 0] == pytest.approx(mu0, rel=1e-13) and st[b, 2] == mu0 and st[b, 3] == mu0
        assert 0.0 <= st[b, 1] <= 2.0 * (n * dc.EPS * mu0) ** 2
    assert st[0, 1] == 0.0 and st[0, 0] == mu0
    h.close()


def test_statistics_of_signed_zero_duplicate_and_extreme_mu(gpu, capi, synth):
    """mu set through eds_depth_set: mixed signs, +-0.0 among the values, 90 % duplicates, one huge and one tiny magnitude — order
    statistics exact against np.sort, mean and variance within 1e-13 / 1e-12 (N up to 16 000)"""
    rng = np.random.default_rng(77)
    rows = []
    for n in (2000, 1999, 16000, 257):
        x = rng.uniform(-0.5, 1.5, size=n); rows.append(x)                                   # mixed signs
    z = rng.uniform(-0.5, 1.5, size=2000); z[rng.choice(2000, 900, replace=False)] = 0.0; z[rng.choice(2000, 700, replace=False)] = -0.0
    rows.append(z)                                                                              # the median and the third are zeros
    z2 = np.where(rng.random(1500) < 0.5, 0.0, -0.0); z2[:3] = (-1.0, 2.5, 0.5); rows.append(z2)
    d = rng.uniform(-0.5, 1.5, size=16000); d[rng.choice(16000, 14400, replace=False)] = 0.4375; rows.append(d)     # 90 % duplicates
    d2 = rng.uniform(0.2, 1.0, size=3000); d2[rng.random(3000) < 0.9] = d2[0]; rows.append(d2)
    e = rng.uniform(-0.5, 1.5, size=2000); e[17] = 1e150; e[1203] = 1e-300; rows.append(e)     # one huge, one tiny
    e2 = rng.uniform(-0.5, 1.5, size=300); e2[5] = -1e150; e2[6] = -5e-324; rows.append(e2)
    als = [dc.alignment(b, len(x)) for b, x in enumerate(rows)]
    h = capi.Handle(_ref12(capi), len(rows), max(len(x) for x in rows), dc.H, dc.W)
    for b, a in enumerate(als):
        h.set_alignment(b, a)
    h.depth_init(0, len(rows), capi.DEPTH_INIT_CONSTANT, min_depth=MIN_D, max_depth=MAX_D)
    for b, x in enumerate(rows):
        s = np.column_stack([x, np.full(len(x), 0.5), np.full(len(x), 2.0), np.full(len(x), 5.0)])
        h.depth_set(b, s)
    st = h.depth_stats()
    for b, x in enumerate(rows):
        m, v, med, third = _stats_want(x)
        print(b, len(x), st[b], (m, v, med, third))
        assert st[b, 0] == pytest.approx(m, rel=1e-13) and st[b, 1] == pytest.approx(v, rel=1e-12)
        assert st[b, 2] == med and st[b, 3] == third
    # a sub-range of the same handle
    assert np.array_equal(h.depth_stats(4, 3), st[4:7])
    h.close()


def test_gauss_filter_runs_vogiatzis(gpu, capi, synth):
    case = dc.make_case("negative_mu_seed", n_slots=4, n0=400)
    res = []
    for filt in (capi.DEPTH_VOGIATZIS, capi.DEPTH_GAUSS):
        h, _ = _case_handle(capi, case, range(4))
        _seed_case(capi, h, case)
        sums = _update_case(capi, h, case, filter=filt)
        res.append((sums, [h.depth_get(b)[0] for b in range(4)]))
        h.close()
    assert res[0][0] == res[1][0] and sum(s["mu_reset"] for s in res[0][0]) > 0
    for x, y in zip(res[0][1], res[1][1]):
        assert np.array_equal(x, y)


def test_depth_set_get_round_trip_on_a_middle_slot(gpu, capi, synth):
    ns = (300, 411, 257, 500, 123)
    als = [dc.alignment(b, n) for b, n in enumerate(ns)]
    h = capi.Handle(_ref12(capi), len(ns), max(ns), dc.H, dc.W)
    for b, a in enumerate(als):
        h.set_alignment(b, a)
    h.depth_init(0, len(ns), capi.DEPTH_INIT_PLANE, min_depth=MIN_D, max_depth=MAX_D)
    before = [h.depth_get(b)[0] for b in range(len(ns))]
    rng = np.random.default_rng(8)
    s = rng.uniform(-2.0, 2.0, size=(257, 4))
    s[:12] = np.array([5e-324, -5e-324, 1e-310, 2.2250738585072014e-308, 1.7976931348623157e308, -1.7976931348623157e308, 1e300, -0.0, 0.0,
                       1e-45, 3.5e38, -1e-200]).reshape(12, 1)
    h.depth_set(2, s)
    got = h.depth_get(2)[0]
    assert np.array_equal(got.view(np.int64), s.view(np.int64))
    assert np.array_equal(h.depth_get_idepth(2).view(np.int64), np.ascontiguousarray(s[:, 0]).view(np.int64))
    for b in (0, 1, 3, 4):
        assert np.array_equal(h.depth_get(b)[0].view(np.int64), before[b].view(np.int64))
    _plane_is_narrowed_mu(capi, h, 2, [dc.Slot(K4=None, kf_xy=None, ef_xy=None, seeds=s)], [s[:, 0]])
    h.close()


def test_set_idepth_leaves_seeds_and_reproject_reads_the_plane(gpu, capi, synth):
    """eds_trk_set_idepth after seeding: seeds stay, the plane changes; the next EDS_DEPTH_REPROJECT tracks with the NEW plane and
    filters the OLD mu; EDS_DEPTH_INIT_PLANE then seeds the narrowed new values"""
    rng = np.random.default_rng(12)
    als = [dc.alignment(b, 500 - 40 * b, seed=9) for b in range(3)]
    h = capi.Handle(_ref12(capi), 3, 500, dc.H, dc.W)
    for b, a in enumerate(als):
        h.set_alignment(b, a)
    mu0 = [a.idp * (1.0 + rng.normal(scale=0.05, size=a.N)) for a in als]
    h.depth_init(0, 3, capi.DEPTH_INIT_HOST, idp=mu0, min_depth=MIN_D, max_depth=MAX_D)
    new = als[1].idp * rng.uniform(0.7, 1.4, size=als[1].N)
    seeds0 = [h.depth_get(b)[0] for b in range(3)]
    h.set_idepth(1, new)
    for b in range(3):
        assert np.array_equal(h.depth_get(b)[0], seeds0[b])
    poses = [_quat_pose(rng) for _ in range(3)]
    h.set_states(0, np.array([p for p, _ in poses]), np.array([q for _, q in poses]), np.zeros((3, 6)))
    got = h.depth_update(0, 3, capi.DEPTH_REPROJECT)
    for b, a in enumerate(als):
        K4 = (a.fx, a.fy, a.cx, a.cy)
        prm = do.Params(do.K_matrix(*K4), MIN_D, MAX_D)
        seeds = seeds0[b].copy()
        kf = do.slot_pixels(a.norm_coord, K4)
        rho = (new if b == 1 else mu0[b]).astype(np.float32)
        want = do.update(prm, seeds, kf, kf + do.reproject_tracks(a.norm_coord, rho, K4, *poses[b]), *do.T_ef_kf_from(p=poses[b][0], q=poses[b][1]))
        assert got[b] == want
        assert _close(h.depth_get(b)[0], seeds)
        if b == 1:      # the old plane would have given other seeds: the test can tell the two apart
            other = seeds0[b].copy()
            do.update(prm, other, kf, kf + do.reproject_tracks(a.norm_coord, mu0[b].astype(np.float32), K4, *poses[b]),
                      *do.T_ef_kf_from(p=poses[b][0], q=poses[b][1]))
            assert not _close(other, seeds, rel=1e-6)
    h.set_idepth(1, new)
    h.depth_init(1, 1, capi.DEPTH_INIT_PLANE, min_depth=MIN_D, max_depth=MAX_D)
    s = h.depth_get(1)[0]
    assert np.array_equal(s[:, 0], new.astype(np.float32).astype(np.float64)) and np.all(s[:, 1] == (MAX_D - MIN_D) ** 2 / 36.0)
    h.close()


def test_sixty_free_running_steps(gpu, capi, synth):
    """the loop on the device for 60 steps (EDS_DEPTH_REPROJECT: plane -> track -> filter -> plane), distinct intrinsics per slot,
    against the oracle after EVERY step.  mu, a and b within REL.  sigma2 within REL or the free run's allowance: the fp64 oracle
    itself leaves REL of sigma2 against extended precision from step 31 on (tests/test_depth_oracle.py::
    test_free_run_allowance_measurement: 3.2e-9, 4.27 units of 2^-52 2 mu^2); the allowance is 4 x that, 17.08 units.  converged is
    compared where sigma2 is further than its tolerance from the threshold."""
    als, idp0, poses = dc.free_run_scene()
    history, planes = dc.free_run_oracle(als, idp0, poses)
    h = _setup(capi, synth, als)
    h.depth_init(0, 2, capi.DEPTH_INIT_HOST, idp=idp0, min_depth=dc.MIN_D, max_depth=dc.MAX_D, threshold=100.0)
    th2 = ((dc.MAX_D - dc.MIN_D) / 100.0) ** 2
    worst = [0.0, 0.0]
    for step, states in enumerate(poses):
        for b in range(2):       # the plane the device is about to read is the one the oracle's step read
            assert np.array_equal(h.depth_get_idepth(b).astype(np.float32), planes[step][b]), (step, b)
        h.set_states(0, np.array([p for p, _ in states]), np.array([q for _, q in states]), np.stack([a.v0 for a in als]))
        sums = h.depth_update(0, 2, capi.DEPTH_REPROJECT)
        for b in range(2):
            want = history[step][b]
            s, conv = h.depth_get(b)
            assert _close(s[:, [0, 2, 3]], want[:, [0, 2, 3]]), (step, b)
            tol = dc.free_run_sigma2_tolerance(want)
            d = np.abs(s[:, 1] - want[:, 1])
            worst = [max(worst[0], float(np.max(d / tol))), max(worst[1], float(np.max(d / want[:, 1])))]
            assert np.all(d <= tol), (step, b, float(np.max(d / tol)), float(np.max(d / want[:, 1])))
            far = np.abs(want[:, 1] - th2) > tol
            assert np.array_equal(conv[far], (want[:, 1] < th2)[far])
            assert sums[b]["updated"] == als[b].N and sums[b]["converged"] == int(conv.sum())
    print(f"max sigma2 difference / tolerance {worst[0]:.3g}, max relative {worst[1]:.3g}")
    h.close()
