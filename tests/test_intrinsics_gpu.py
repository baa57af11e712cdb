"""The tracker core under cameras that are NOT symmetric in x and y (tests/intrinsics_cases.py): fx != fy, the principal point several
pixels off the centre, portrait and landscape frames, keyframe pixels off the grid, on the border and just outside it.  Under
synth.intrinsics (fx == fy, centred) a kernel may take fx for fy, cx for cy or W for H and the rest of the suite still passes; here every
place where the camera enters — rows, the persistent kernels by code family, point maintenance, the three upload paths, build_keyframe,
the pyramid, the mirrors — is compared with the oracles at the project's own tolerances:

    rows             tests/test_parity_gpu.py      TOL_R 1e-5, TOL_J = TOL_H 1e-4, TOL_STEP = TOL_POSE 1e-4
    persistent       tests/test_instances_gpu.py   accept pattern / step counts equal, pose 1e-6 (bicubic) / 1e-4 (bilinear), residuals 1e-5
    points           tests/test_points_gpu.py      kept exact, 5e-5 px, 1e-5 relative flow

tests/test_intrinsics_oracle.py shows on the CPU that these inputs tell fx from fy by 100 x the residual tolerance and more."""
import importlib

import numpy as np
import pytest

import intrinsics_cases as ic
import subpixel_cases as sc

pytestmark = pytest.mark.gpu

TOL_R, TOL_J, TOL_H, TOL_STEP, TOL_POSE = 1e-5, 1e-4, 1e-4, 1e-4, 1e-4
_id = lambda c: f"{c[0]}-{c[1]}x{c[2]}"
_key = lambda k: "-".join(map(str, k))


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def _handle(capi, al, batch=1, **kw):
    h = capi.Handle(capi.default_config(**kw), batch, al.N, al.H, al.W)
    for b in range(batch):
        h.set_alignment(b, al)
    return h


def _check_rows(capi, po, h, al, p, q, v, sampling, nb, nc, tag):
    """r, J, JtJ, Jtr and the cost of eval with 6 and 12 columns against the oracle; prints the figures it asserts"""
    o = po.Oracle(al, sampling=sampling, num_blocks=nb, nc=nc)
    out = []
    if not nc:
        g, e = h.eval(0, p, q, v, ncols=6), o.pose6_eval(p, q, v)                   # (the model is normalised per block there too)
        out.append(("6", np.abs(g["r"] - e["r"]).max() / np.abs(e["r"]).max(), rel(g["J"], e["J"]), rel(g["JtJ"], e["H"]), rel(g["Jtr"], e["b"]),
                    abs(g["cost"] / (0.5 * e["cost"]) - 1.0)))
        assert np.array_equal(g["JtJ"], g["JtJ"].T)
    g, e = h.eval(0, p, q, v, ncols=12), o.eval12(p, q, v)
    J, r = e["J_local_raw"], e["r_raw"]
    out.append(("12", np.abs(g["r"] - r).max() / np.abs(r).max(), rel(g["J"], J), rel(g["JtJ"], J.T @ J), rel(g["Jtr"], J.T @ r),
                abs(g["cost"] / (0.5 * np.sum(r * r)) - 1.0)))
    for cols, dr, dj, dh, db, dc in out:
        print(f"[rows] {tag} ncols={cols}: |dr|/max|r| {dr:.2e}  J {dj:.2e}  JtJ {dh:.2e}  Jtr {db:.2e}  cost {dc:.2e}")
    for cols, dr, dj, dh, db, dc in out:
        assert dr <= TOL_R and dj <= TOL_J and dh <= TOL_H and db <= TOL_H and dc <= 1e-5, (tag, cols, dr, dj, dh, db, dc)


# ---- rows (the host-driven kernels) -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ic.ROW_CASES, ids=_id)
def test_rows_vs_oracle(gpu, capi, po, npo, case):
    """eval with 6 and 12 columns, both samplers, one and three blocks, the plain and the NC residual, on 300 sub-pixel points plus
    EDGE_PIXELS; once more from the strip copies of the frame; on portrait frames once more at a pose that throws a quarter of the
    points out of the frame."""
    cam, H, W = case
    al = ic.row_alignment(cam, H, W)
    raw = ic.replace(al, frame=al.frame * 37.5)                          # the NC functor takes the frame un-normalised
    p, q = ic.eval_pose()
    v = al.v_true
    for sampling in (0, 1):
        for nb in (1, 3):
            for nc in (False, True):
                a = raw if nc else al
                h = _handle(capi, a, sampling=sampling, num_blocks=nb, nc=int(nc), exec=capi.EXEC_HOST,
                            solver=capi.SOLVER_REF12 if nc else capi.SOLVER_LM6)
                tag = f"{cam} {H}x{W} {'bicubic' if sampling == 0 else 'bilinear'} nb={nb}{' NC' if nc else ''}"
                _check_rows(capi, po, h, a, p, q, v, sampling, nb, nc, tag)
                if sampling == 0 and nb == 1 and not nc:
                    h.prepare_frames(0, 1)                               # eval reads the strip copies once they are current
                    assert not h.strips_info()["unavailable"] and h.strips_info()["bytes"] > 0
                    _check_rows(capi, po, h, a, p, q, v, sampling, nb, nc, tag + " strips")
                if nb == 1 and not nc and H > W:
                    _, _, uu, vv = npo.project(a, ic.P_OUT, ic.Q_OUT())
                    outside = ((uu < 0) | (uu > W - 1) | (vv < 0) | (vv > H - 1)).mean()
                    assert 0.2 < outside < 0.85, outside
                    _check_rows(capi, po, h, a, ic.P_OUT, ic.Q_OUT(), v, sampling, nb, nc, tag + f" {outside:.0%} outside")
                h.close()


def test_rows_davis(gpu, capi, po):
    """the DAVIS-like camera (fy / fx = 0.9987): parity only, it cannot tell fx from fy at these tolerances"""
    for H, W in (ic.PORTRAIT, (120, 160)):
        al = ic.row_alignment("davis", H, W)
        p, q = ic.eval_pose()
        for sampling in (0, 1):
            h = _handle(capi, al, sampling=sampling, num_blocks=3, exec=capi.EXEC_HOST)
            _check_rows(capi, po, h, al, p, q, al.v_true, sampling, 3, False, f"davis {H}x{W} sampler {sampling}")
            h.close()


# ---- the persistent kernels, one launch family per test --------------------------------------------------------------------------------
def _upload(h, als):
    for b, a in enumerate(als):
        h.set_keyframe(b, a.norm_coord, a.grad, a.idp, a.weights, a.fx, a.fy, a.cx, a.cy)
        h.set_event_frame(b, np.ascontiguousarray(a.frame, dtype=np.float32))      # (the cases' frames are fp32 values already)
    B = len(als)
    h.set_states(0, np.stack([ic.PS] * B), np.stack([ic.QS()] * B), np.stack([a.v0 for a in als]))


def _check_lm6(capi, po, h, als, S, tau, tag, tol=None):
    """tests/test_instances_gpu.py's assertions on an LM6 batch that has been solved"""
    tab = h.results(0, len(als))
    worst = 0.0
    for b, a in enumerate(als):
        o = po.Oracle(a, sampling=S)
        ref = o.pose6_lm(ic.PS, ic.QS(), a.v0, iters=ic.SOLVE_ITERS, lambda0=h.get_config().lambda0, huber_tau=tau)
        acc = h.trace(b)["accepted"]
        assert tab[b, 15] == 1.0 and tab[b, 14] == ref["iterations"], (tag, b)
        assert np.array_equal(acc, ref["accepted"]), (tag, b, acc, ref["accepted"])
        d = po.se3_distance(tab[b, 0:3], tab[b, 3:7], ref["p"], ref["q"])
        worst = max(worst, d)
        assert d <= (tol if tol is not None else (1e-6 if S == 0 else 1e-4)), (tag, b, d)
        if b == 0 and S == 0:
            er = o.pose6_eval(tab[b, 0:3], tab[b, 3:7], a.v0, huber_tau=0.0)["r"]
            assert np.abs(h.residuals(b) - er).max() <= 1e-5 * np.abs(er).max(), tag
    print(f"[solve] {tag}: pose distance to the oracle {worst:.2e}")


@pytest.mark.parametrize("fam", ic.FUSED6_FAMILIES, ids=_key)
def test_fused6_family_vs_oracle(gpu, capi, po, fam):
    """The first instantiation of one (S, Q, K > 1, G > 1) family of eds_fused6_kernel, launched by name on a batch of three `tall`
    alignments on a portrait frame."""
    S, P, T, Q, K, G = ic.first_of_each(capi.kernel_instances(0), ic.fused6_family)[fam]
    huber = Q in (2, 4)
    tau = ic.SOLVE_TAU if huber else 0.0
    N = ic.fused6_points((S, P, T, Q, K, G))
    als = ic.solve_case(("lm6", N, S, int(huber)))
    H, W = ic.solve_frame(N)
    cfg = capi.default_config(sampling=S, solver=capi.SOLVER_LM6, exec=capi.EXEC_DEVICE, max_num_iterations=ic.SOLVE_ITERS, huber_tau=tau)
    h = capi.Handle(cfg, ic.SOLVE_B, N, H, W)
    _upload(h, als)
    if Q >= 3:
        h.prepare_frames(0, ic.SOLVE_B)
    h.set_knob("EDS_FORCE_FUSED6", f"{S},{P},{T},{Q},{K},{G}")
    h.optimize_batch(0, 0, ic.SOLVE_B)
    want = f"eds_fused6_kernel<{S}, {P}, {T}, {Q}, {K}" + (f", {G}>" if G > 1 else ">")
    assert h.last_launch()["kernel"] == want, (h.last_launch()["kernel"], want)
    assert h.info(0)["flags"] == 0, "team time-out"
    _check_lm6(capi, po, h, als, S, tau, f"{want} {H}x{W} N={N}")
    h.close()


def _check_ref12(capi, po, h, als, S, NC, tag, kw):
    tab = h.results(0, len(als))
    worst = 0.0
    for b, a in enumerate(als):
        o = po.Oracle(a, sampling=S, nc=bool(NC), loss_type=po.LOSS_HUBER, max_num_iterations=ic.SOLVE_ITERS, **kw)
        ref = o.solve_lm(ic.PS, ic.QS(), a.v0)
        info = h.info(b)
        assert info["success"] and (info["num_successful_steps"], info["num_unsuccessful_steps"]) == \
            (ref["num_successful_steps"], ref["num_unsuccessful_steps"]), (tag, b, info, ref)
        assert info["termination"] == ref["termination"], (tag, b)
        if S == 1 and NC:
            # tests/test_instances_gpu.py: bilinear AND NC is checked by function value, 1e-4, not by trajectory
            er = o.eval12(tab[b, 0:3], tab[b, 3:7], tab[b, 7:13], jac=False)["r_raw"]
            assert np.abs(h.residuals(b) - er).max() <= 1e-4 * np.abs(er).max(), (tag, b)
        else:
            tol = 1e-6 if S == 0 else 1e-4
            d, dv = po.se3_distance(tab[b, 0:3], tab[b, 3:7], ref["p"], ref["q"]), np.abs(tab[b, 7:13] - ref["v"]).max()
            worst = max(worst, d, dv)
            assert d <= tol and dv <= tol, (tag, b, d, dv)
    print(f"[solve] {tag}: pose / velocity distance to the oracle {worst:.2e}")


def _run_fused12(capi, po, inst, G):
    S, T, CAP, NC, K, Q = inst
    N = ic.fused12_points(K, G)
    als = ic.solve_case(("ref12", N, S, NC))
    H, W = ic.solve_frame(N)
    cfg = capi.default_config(sampling=S, solver=capi.SOLVER_REF12, exec=capi.EXEC_DEVICE, max_num_iterations=ic.SOLVE_ITERS, nc=NC,
                              loss_type=capi.LOSS_HUBER, **ic.REF12_KW)
    h = capi.Handle(cfg, ic.SOLVE_B, N, H, W)
    _upload(h, als)
    if Q == 2:
        h.prepare_frames(0, ic.SOLVE_B)
    h.set_knob("EDS_FORCE_FUSED12", f"{S},{T},{CAP},{NC},{K},{Q}")
    h.set_knob("EDS_REF12_GROUPS", str(G))
    h.optimize_batch(0, 0, ic.SOLVE_B)
    want = f"eds_fused12_kernel<{S}, {T}, {CAP if G == 1 else 512}, {'true' if NC else 'false'}, {K}, {Q}" + (f", {G}>" if G > 1 else ">")
    assert h.last_launch()["kernel"] == want, (h.last_launch()["kernel"], want)
    assert h.info(0)["flags"] == 0, "team time-out"
    _check_ref12(capi, po, h, als, S, NC, f"{want} {H}x{W} N={N}", ic.REF12_KW)
    h.close()


@pytest.mark.parametrize("fam", ic.FUSED12_FAMILIES, ids=_key)
def test_fused12_family_vs_oracle(gpu, capi, po, fam):
    """The first instantiation of one (S, NC, Q, K > 1) family of eds_fused12_kernel, launched by name."""
    inst = ic.first_of_each(capi.kernel_instances(1), ic.fused12_family)[fam]
    assert inst[2] not in (2000, 736)                                   # (the slim one-block shapes are no family's first instantiation)
    _run_fused12(capi, po, inst, 1)


@pytest.mark.parametrize("grp", ic.FUSED12_GROUPS, ids=_key)
def test_fused12_candidate_groups_vs_oracle(gpu, capi, po, grp):
    """One entry of the candidate-group list {S, T, NC, K, Q, G}: the one-team instantiation it extends, forced, with G groups."""
    assert grp in capi.kernel_instances(2)
    S, T, NC, K, Q, G = grp
    _run_fused12(capi, po, (S, T, 1408, NC, K, Q), G)


def test_families_cover_the_library(gpu, capi):
    """The literal family lists of tests/intrinsics_cases.py are what the library's own lists give today: a family added to the
    library without a case here fails this test."""
    f6 = list(ic.first_of_each(capi.kernel_instances(0), ic.fused6_family))
    f12 = list(ic.first_of_each(capi.kernel_instances(1), ic.fused12_family))
    assert f6 == ic.FUSED6_FAMILIES and f12 == ic.FUSED12_FAMILIES and capi.kernel_instances(2) == ic.FUSED12_GROUPS
    n = len(f6) + len(f12) + len(ic.FUSED12_GROUPS)
    print(f"\n[families] {len(f6)} eds_fused6_kernel + {len(f12)} eds_fused12_kernel + {len(ic.FUSED12_GROUPS)} candidate-group families = {n} "
          "launched by name under the tall camera")
    assert n == 43


@pytest.mark.parametrize("kernel", ["resident", "paired", "wide"])
def test_lm6_kernel_knob_vs_oracle(gpu, capi, po, kernel):
    """EDS_LM6_KERNEL = resident / paired / wide (the register-resident kernel and both shapes of eds_stream6_kernel), with and
    without per-point Huber weights: tests/test_parity_gpu.py's assertions (accept pattern, pose 1e-4, kept residuals)."""
    for huber in (0, 1):
        tau = ic.SOLVE_TAU if huber else 0.0
        als = ic.solve_case(("lm6", 1011, 0, huber))
        H, W = ic.solve_frame(1011)
        cfg = capi.default_config(solver=capi.SOLVER_LM6, exec=capi.EXEC_DEVICE, max_num_iterations=ic.SOLVE_ITERS, huber_tau=tau)
        h = capi.Handle(cfg, ic.SOLVE_B, 1011, H, W)
        h.set_knob("EDS_LM6_KERNEL", kernel)
        _upload(h, als)
        h.optimize_batch(0, 0, ic.SOLVE_B)
        name = h.last_launch()["kernel"]
        assert ("eds_stream6_kernel" in name) == (kernel != "resident"), name
        _check_lm6(capi, po, h, als, 0, tau, f"EDS_LM6_KERNEL={kernel} tau={tau}: {name}", tol=TOL_POSE)
        h.close()


@pytest.mark.parametrize("solver", ["lm6", "lm6-huber", "gn6", "ref12"])
def test_host_loop_vs_oracle(gpu, capi, po, solver):
    """EXEC_HOST: the streaming row kernels and the reduction driven from the host, under `tall` on a portrait frame."""
    if solver == "ref12":
        al = ic.solve_case(("ref12", 2000, 0, 0))[0]
        h = _handle(capi, al, exec=capi.EXEC_HOST, solver=capi.SOLVER_REF12, loss_type=capi.LOSS_HUBER, max_num_iterations=ic.SOLVE_ITERS, **ic.REF12_KW)
        h.set_state(0, ic.PS, ic.QS(), al.v0)
        h.optimize_batch(0, 0, 1)
        _check_ref12(capi, po, h, [al], 0, 0, "host loop REF12", ic.REF12_KW)
    elif solver == "gn6":
        al = ic.solve_case(("lm6", 1011, 0, 0))[0]
        h = _handle(capi, al, exec=capi.EXEC_HOST, solver=capi.SOLVER_GN6, max_num_iterations=3)
        p, q, _, info = h.optimize(0, p=ic.PS, q=ic.QS(), v=al.v0)
        ref = po.Oracle(al).pose6_gn(ic.PS, ic.QS(), al.v0, iters=3)
        tr = h.trace(0)
        assert info["num_iterations"] == 3 and len(tr["increments"]) == 3
        ta, qa = po.se3_exp(tr["increments"][0])
        tb, qb = po.se3_exp(ref["increments"][0])
        assert po.se3_distance(ta, qa, tb, qb) / max(np.linalg.norm(ref["increments"][0]), 1e-3) <= TOL_STEP
        assert po.se3_distance(p, q, ref["p"], ref["q"]) <= TOL_POSE
    else:
        huber = int(solver == "lm6-huber")
        tau = ic.SOLVE_TAU if huber else 0.0
        al = ic.solve_case(("lm6", 1011, 0, huber))[0]
        h = _handle(capi, al, exec=capi.EXEC_HOST, solver=capi.SOLVER_LM6, max_num_iterations=ic.SOLVE_ITERS, huber_tau=tau)
        h.set_state(0, ic.PS, ic.QS(), al.v0)
        h.optimize_batch(0, 0, 1)
        _check_lm6(capi, po, h, [al], 0, tau, f"host loop LM6 tau={tau}", tol=TOL_POSE)
    h.close()


def test_lm6_davis(gpu, capi, po):
    als = ic.solve_case(("lm6", 499, 0, 0), cam="davis")
    cfg = capi.default_config(solver=capi.SOLVER_LM6, exec=capi.EXEC_DEVICE, max_num_iterations=ic.SOLVE_ITERS)
    h = capi.Handle(cfg, ic.SOLVE_B, 499, *ic.solve_frame(499))
    _upload(h, als)
    h.optimize_batch(0, 0, ic.SOLVE_B)
    _check_lm6(capi, po, h, als, 0, 0.0, "davis LM6 " + h.last_launch()["kernel"])
    h.close()


# ---- point maintenance ------------------------------------------------------------------------------------------------------------------
def _points_ref(al, p, q, delete=True):
    import np_points_oracle as pto
    return pto.get_coord(al.norm_coord, al.idp, al.coord, (al.fx, al.fy, al.cx, al.cy), al.H, al.W, p, q, delete)


def _check_points(out, ref, tag):
    assert np.array_equal(out["kept"], ref["kept"]), tag
    dc, dt = np.abs(out["coord"] - ref["coord"]).max(), np.abs(out["tracks"] - ref["tracks"]).max()
    df = abs(out["mean_sq_flow"] / ref["mean_sq_flow"] - 1.0)
    print(f"[points] {tag}: coord {dc:.2e} px  tracks {dt:.2e} px  mean_sq_flow {df:.2e}")
    assert dc < 5e-5 and dt < 5e-5 and df <= 1e-5, (tag, dc, dt, df)


def _kept(al, keep):
    return ic.replace(al, **{k: getattr(al, k)[keep] for k in ("norm_coord", "grad", "idp", "weights", "coord")})


@pytest.mark.parametrize("cam", ic.DISCRIMINATING)
@pytest.mark.parametrize("H,W", [ic.PORTRAIT, ic.LANDSCAPE], ids=["portrait", "landscape"])
def test_update_points_vs_oracle(gpu, capi, po, cam, H, W):
    """Tracker::getCoord(true) on 900 sub-pixel points, two of which project between min(H, W) and max(H, W) along one axis (an
    exchange of rows and cols changes which of them is erased); the compacted planes then evaluate like a fresh upload."""
    al = ic.points_alignment(61, H, W, 900, cam)
    p, q = ic.P_PTS, ic.Q_PTS()
    ref = _points_ref(al, p, q)
    assert 30 < al.N - len(ref["kept"]) < al.N - 30
    assert ((al.N - 2 in ref["kept"]), (al.N - 1 in ref["kept"])) == ((False, True) if H > W else (True, False))
    h = capi.Handle(capi.default_config(exec=capi.EXEC_HOST), 1, al.N, H, W)
    h.set_alignment(0, al)
    h.set_state(0, p, q, al.v0)
    _check_points(h.update_points(0, True), ref, f"{cam} {H}x{W}")
    al2 = _kept(al, ref["kept"])
    pe, qe = ic.eval_pose(5)
    g, e = h.eval(0, pe, qe, al.v0, ncols=6), po.Oracle(al2).pose6_eval(pe, qe, al.v0)
    assert g["r"].shape == (len(ref["kept"]),)
    assert np.abs(g["r"] - e["r"]).max() <= TOL_R * np.abs(e["r"]).max() and rel(g["JtJ"], e["H"]) <= TOL_H
    out = h.update_points(0, False)                                     # delete_out_points = false keeps everything
    assert len(out["kept"]) == len(ref["kept"])
    h.close()


@pytest.mark.parametrize("cam", ic.DISCRIMINATING)
def test_update_points_batch_vs_oracle(gpu, capi, po, cam):
    """eds_trk_update_points_batch on a portrait frame: 70 ragged slots (more than one launch of 64) and one slot of 4 097 points
    (more than one sweep of 4 096), each pair of exchange points among them."""
    H, W = ic.PORTRAIT
    rng = np.random.default_rng(17)
    pairs = []
    for k in range(8):
        p = ic.P_PTS * rng.uniform(1.0, 3.0, 3) * np.where(rng.uniform(size=3) < 0.5, -1.0, 1.0)
        q = importlib.import_module("slam-eds_amd.synth").quat_from_axis_angle(rng.standard_normal(3), 0.05 * rng.uniform(0.2, 1.0))
        al = ic.points_alignment(700 + k, H, W, int(rng.integers(64, 900)), cam, p, q)
        pairs.append((al, p, q, _points_ref(al, p, q)))
    big = ic.points_alignment(790, H, W, 4097, cam)
    pairs.append((big, ic.P_PTS, ic.Q_PTS(), _points_ref(big, ic.P_PTS, ic.Q_PTS())))
    B = 71
    slots = [pairs[b % 8] for b in range(70)] + [pairs[8]]
    h = capi.Handle(capi.default_config(exec=capi.EXEC_HOST), B + 2, 4097, H, W)
    for b, (al, p, q, _) in enumerate(slots):
        h.set_alignment(1 + b, al)
        h.set_state(1 + b, p, q, al.v0)
    h.set_alignment(0, pairs[0][0]); h.set_alignment(B + 1, pairs[1][0])       # neighbours that must stay as they are
    outs = h.update_points_batch(1, B, True)
    erased = 0
    for b, (al, p, q, ref) in enumerate(slots):
        assert outs[b]["n"] == len(ref["kept"]), b
        assert ((al.N - 2 in ref["kept"]), (al.N - 1 in ref["kept"])) == (False, True)
        erased += al.N - outs[b]["n"]
        if b in (0, 3, 7, 64, 69, 70):
            _check_points(outs[b], ref, f"{cam} slot {b} N={al.N}")
        else:
            assert np.array_equal(outs[b]["kept"], ref["kept"]) and np.abs(outs[b]["coord"] - ref["coord"]).max() < 5e-5
            assert np.abs(outs[b]["tracks"] - ref["tracks"]).max() < 5e-5 and abs(outs[b]["mean_sq_flow"] / ref["mean_sq_flow"] - 1) <= 1e-5
    assert erased > 100
    pe, qe = ic.eval_pose(5)
    for b in (0, 69, 70):
        al, _, _, ref = slots[b]
        al2 = _kept(al, ref["kept"])
        g, e = h.eval(1 + b, pe, qe, al.v0, ncols=6), po.Oracle(al2).pose6_eval(pe, qe, al.v0)
        assert np.abs(g["r"] - e["r"]).max() <= TOL_R * np.abs(e["r"]).max() and rel(g["JtJ"], e["H"]) <= TOL_H
    for s_, al in ((0, pairs[0][0]), (B + 1, pairs[1][0])):
        assert h.update_points(s_, False)["coord"].shape[0] == al.N
    h.close()


# ---- the three upload paths -------------------------------------------------------------------------------------------------------------
def test_upload_paths_agree_bit_for_bit(gpu, capi):
    """set_keyframe, set_keyframes_device for one slot and for a range of slots (a camera of its own per slot) leave the same planes:
    the same eval rows and the same LM6 result, bit for bit, under `tall` with sub-pixel points and EDGE_PIXELS."""
    H, W = ic.PORTRAIT
    al = ic.solve_case(("lm6", 499, 0, 0))[0]
    others = [ic.row_alignment("wide", H, W), ic.row_alignment("davis", H, W)]
    S = al.N + 5
    cfg = capi.default_config(solver=capi.SOLVER_LM6, exec=capi.EXEC_DEVICE, max_num_iterations=ic.SOLVE_ITERS)
    h = capi.Handle(cfg, 5, al.N, H, W)

    def dev(als_):
        pack = lambda rows: np.ascontiguousarray(np.stack([np.concatenate([r, np.full((S - len(r),) + r.shape[1:], 9e9)]) for r in rows]))
        return [capi.DeviceArray.from_numpy(pack([getattr(a, n) for a in als_])) for n in ("norm_coord", "grad", "idp", "weights")]

    Kof = lambda a: [a.fx, a.fy, a.cx, a.cy]
    h.set_keyframe(0, al.norm_coord, al.grad, al.idp, al.weights, *Kof(al))
    one = dev([al])
    h.set_keyframes_device(1, [al.N], *one, np.array([Kof(al)]))
    rng_als = [others[0], al, others[1]]
    three = dev(rng_als)
    h.set_keyframes_device(2, [a.N for a in rng_als], *three, np.array([Kof(a) for a in rng_als]))
    h.set_event_frames(0, [al.frame] * 5)
    p, q = ic.eval_pose()
    ref_rows, ref_solve = None, None
    for slot in (0, 1, 3):
        rows = [h.eval(slot, p, q, al.v0, ncols=n) for n in (6, 12)]
        pg, qg, _, info = h.optimize(slot, p=ic.PS, q=ic.QS(), v=al.v0)
        solve = (pg, qg, h.trace(slot)["accepted"], h.residuals(slot))
        if ref_rows is None:
            ref_rows, ref_solve = rows, solve
            assert (solve[2] == 0).any() and (solve[2] == 1).any()
            continue
        for a, b in zip(rows, ref_rows):
            for k in ("r", "J", "JtJ", "Jtr"):
                assert np.array_equal(a[k], b[k]), (slot, k)
            assert a["cost"] == b["cost"]
        assert all(np.array_equal(x, y) for x, y in zip(solve, ref_solve)), slot
    h.sync()
    h.close()


# ---- build_keyframe ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [False, True], ids=["no-depth", "depth-map"])
def test_build_keyframe_under_tall(gpu, capi, po, depth):
    """One u8 image at (83, 61): norm_coord and coord as np_keyframe_oracle computes them, and the slot then evaluates like one filled
    by set_keyframe with the returned arrays."""
    import np_keyframe_oracle as ko
    import test_keyframe as tk
    H, W = ic.PORTRAIT
    K = ic.camera("tall", H, W)
    img = tk.make_image(17, H, W)
    xy, di = tk.make_depth_map(18, H, W, 400) if depth else (None, None)
    ref = ko.keyframe(img, K, ko.MEDIAN, 0, depth_xy=xy, depth_idp=di)
    h = capi.Handle(capi.default_config(exec=capi.EXEC_HOST), 2, H * W, H, W)
    out = h.build_keyframe(0, img, K, method=capi.KF_MEDIAN, depth_xy=xy, depth_idp=di)
    tk._compare(out, ref)
    N = len(out["idp"])
    assert N > 300 and np.array_equal(out["norm_coord"], np.column_stack([(out["coord"][:, 0] - K[2]) / K[0], (out["coord"][:, 1] - K[3]) / K[1]]))
    h.set_keyframe(1, out["norm_coord"], out["grad"], out["idp"], out["weights"], *K)
    frame = ic.row_alignment("tall", H, W).frame
    for s in (0, 1):
        h.set_event_frame(s, frame)
    p, q = ic.eval_pose()
    v = ic.row_alignment("tall", H, W).v_true
    a, b = h.eval(0, p, q, v, ncols=12), h.eval(1, p, q, v, ncols=12)
    assert np.array_equal(a["r"], b["r"]) and np.array_equal(a["J"], b["J"]) and np.array_equal(a["JtJ"], b["JtJ"])
    al2 = ic.replace(ic.row_alignment("tall", H, W), norm_coord=out["norm_coord"], grad=out["grad"], idp=out["idp"], weights=out["weights"],
                     coord=out["coord"])
    e = po.Oracle(al2).eval12(p, q, v)
    assert np.abs(a["r"] - e["r_raw"]).max() <= TOL_R * np.abs(e["r_raw"]).max()
    h.close()


# ---- the pyramid ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["lm6", "ref12"])
def test_pyramid_under_tall(gpu, capi, po, solver):
    """capi.Pyramid with 3 levels from (160, 120), 1 200 / 600 / 300 points with pixels on row 0 and column 0 among the first 300 (they
    are negative at levels 1 and 2), single and as a batch of three: tests/test_pyramid.py's assertions against np_pyramid_oracle."""
    import np_pyramid_oracle as pyo
    synth = importlib.import_module("slam-eds_amd.synth")
    counts, iters, H, W = ic.PYR_COUNTS, ic.PYR_ITERS, ic.PYR_H, ic.PYR_W
    als = [ic.pyramid_alignment(s) for s in ic.PYR_SEEDS]
    if solver == "lm6":
        cfg, okw = capi.default_config(solver=capi.SOLVER_LM6, exec=capi.EXEC_DEVICE, max_num_iterations=6), {}
    else:
        cfg = capi.default_config(solver=capi.SOLVER_REF12, exec=capi.EXEC_DEVICE, max_num_iterations=6, loss_type=capi.LOSS_HUBER, **ic.PYR_REF12_KW)
        okw = dict(loss_type=po.LOSS_HUBER, **ic.PYR_REF12_KW)
    pb = capi.Pyramid(cfg, counts, H, W, batch=len(als))
    singles = []
    for b, al in enumerate(als):
        one = capi.Pyramid(cfg, counts, H, W)
        for l, n in enumerate(counts):
            pb.set_keyframe_slot(b, l, al.norm_coord[:n], al.grad[:n], al.idp[:n], al.weights[:n], al.fx, al.fy, al.cx, al.cy)
            one.set_keyframe(l, al.norm_coord[:n], al.grad[:n], al.idp[:n], al.weights[:n], al.fx, al.fy, al.cx, al.cy)
        pb.set_event_frame_slot(b, al.frame)
        one.set_event_frame(al.frame)
        singles.append(one.optimize(al.p0, al.q0, al.v0))
        if b == 0:
            assert one.residuals(0).shape == (counts[0],)
        one.close()
    P, Q, V, infos = pb.optimize_batch(np.stack([a.p0 for a in als]), np.stack([a.q0 for a in als]), np.stack([a.v0 for a in als]))
    for b, al in enumerate(als):
        sp, sq, sv, sinfo = singles[b]
        rp, rq, rv, per = pyo.track(po, synth, al, counts, iters, solver=solver, **okw)
        d, dv = po.se3_distance(sp, sq, rp, rq), np.abs(sv - rv).max()
        print(f"[pyramid] {solver} pyramid {b}: pose {d:.2e}  velocity {dv:.2e} from the oracle's track")
        assert d <= 1e-4 and dv <= 1e-4, (b, d, dv)
        assert po.se3_distance(P[b], Q[b], sp, sq) <= 1e-9, b
        for l in range(len(counts)):
            assert infos[l][b]["num_iterations"] == sinfo[l]["num_iterations"] and infos[l][b]["num_points"] == counts[l]
            if solver == "lm6":
                assert sinfo[l]["num_iterations"] == per[l]["iterations"] and sinfo[l]["num_successful_steps"] == int(per[l]["accepted"].sum())
            else:
                assert sinfo[l]["num_iterations"] == per[l]["num_iterations"] and sinfo[l]["num_successful_steps"] == per[l]["num_successful_steps"]
                assert sinfo[l]["termination"] == per[l]["termination"]
        assert po.se3_distance(sp, sq, al.p_true, al.q_true) < po.se3_distance(al.p0, al.q0, al.p_true, al.q_true)
    pb.close()
    fx, fy, cx, cy = ic.camera("tall", H, W)
    for l in range(len(counts)):
        assert np.array_equal(capi.Pyramid.level_intrinsics(l, fx, fy, cx, cy), np.array(pyo.level_intrinsics(l, fx, fy, cx, cy)))


# ---- the mirrors ------------------------------------------------------------------------------------------------------------------------
def test_tracker_mirror_under_tall(gpu, capi, po):
    """tracker.Tracker / KeyFrame with the K matrix of `tall` on a portrait frame: optimize, getCoord(true), needNewKeyframe against
    the oracles (tests/test_parity_gpu.py's and tests/test_points_gpu.py's mirror tests)."""
    import np_points_oracle as pto
    trk = importlib.import_module("slam-eds_amd.tracker")
    al = ic.solve_case(("ref12", 2000, 0, 0))[0]
    K = np.array([[al.fx, 0, al.cx], [0, al.fy, al.cy], [0, 0, 1.0]])
    kf = trk.KeyFrame(al.norm_coord.copy(), al.grad.copy(), al.weights.copy(), al.idp.copy(), K, al.H, al.W)
    cfg = trk.Config(loss_type=trk.HUBER, loss_params=[0.3], options=trk.SolverOptions(num_threads=2, max_num_iterations=[ic.SOLVE_ITERS]))
    t = trk.Tracker(kf, cfg)
    ok, T = t.optimize(0, al.frame, np.eye(4), px=ic.PS, qx=ic.QS(), vx=al.v0, loss_param_method=trk.MAD)
    ref = po.Oracle(al, loss_type=po.LOSS_HUBER, max_num_iterations=ic.SOLVE_ITERS, **ic.REF12_KW).solve_lm(ic.PS, ic.QS(), al.v0)
    assert ok and t.getInfo().success and t.getInfo().num_iterations == ref["num_iterations"]
    assert po.se3_distance(t.px, t.qx, ref["p"], ref["q"]) <= TOL_POSE
    assert np.allclose(T @ t.getTransform(), np.eye(4), atol=1e-12)
    r_fin = po.Oracle(al, num_blocks=2).eval12(ref["p"], ref["q"], ref["v"], jac=False)["r_raw"]
    assert t.config.loss_params[0] == pytest.approx(po.loss_param(r_fin, po.LP_MAD)[0], rel=1e-3)
    t.close()
    # getCoord(true) / needNewKeyframe, with the exchange points
    H, W = ic.PORTRAIT
    pa = ic.points_alignment(63, H, W, 400, "tall")
    K = np.array([[pa.fx, 0, pa.cx], [0, pa.fy, pa.cy], [0, 0, 1.0]])
    kf = trk.KeyFrame(pa.norm_coord.copy(), pa.grad.copy(), pa.weights.copy(), pa.idp.copy(), K, H, W)
    t = trk.Tracker(kf, trk.Config())
    t.reset(kf, ic.P_PTS, ic.Q_PTS(), True)
    ref = _points_ref(pa, ic.P_PTS, ic.Q_PTS())
    coord = t.getCoord(True)
    assert coord.shape == ref["coord"].shape and np.abs(coord - ref["coord"]).max() < 5e-5
    assert np.array_equal(kf.inv_depth, pa.idp[ref["kept"]]) and 0 < len(ref["kept"]) < pa.N
    assert t.squared_norm_flow == pytest.approx(ref["mean_sq_flow"], rel=1e-5)
    for wf in (0.03, 1.0 / max(np.sqrt(ref["mean_sq_flow"]) * 1.05, 1e-9), 1.0 / max(np.sqrt(ref["mean_sq_flow"]) * 0.95, 1e-9)):
        assert t.needNewKeyframe(wf) == pto.need_new_keyframe(ref["mean_sq_flow"], H, W, wf)
    t.close()


def test_cpp_shim_under_tall(gpu, capi, po, tmp_path):
    """tests/test_cpp_shim_gpu.py's driver with the `tall` camera of a portrait frame written into its input file."""
    import test_cpp_shim_gpu as shim
    synth = importlib.import_module("slam-eds_amd.synth")
    al = ic.camera_alignment(808, 320, 240, 700, "tall", pixels="subpixel", start="ctor")
    shim.shim_case(capi, synth, po, tmp_path, al, 4, 1)


def test_epiline_model_image_under_tall(gpu, capi):
    """epi_get_model at (83, 61) under `tall`, sub-pixel points and EDGE_PIXELS, against the epiline oracle's model image."""
    H, W = ic.PORTRAIT
    al = ic.row_alignment("tall", H, W)
    h = capi.Handle(capi.default_config(solver=capi.SOLVER_LM6, exec=capi.EXEC_DEVICE, max_num_iterations=4), 1, al.N, H, W)
    h.set_alignment(0, al)
    h.set_state(0, al.p0, al.q0, sc.VEL)
    got, ref = h.epi_get_model(0), sc.oracle_model(al)
    err = np.abs(got - ref).max()
    print(f"[epiline] model image {H}x{W} under tall: max|got - ref| = {err:.3e}, max|ref| = {np.abs(ref).max():.3e}")
    assert np.abs(ref).max() > 0 and err <= 1e-12 * np.abs(ref).max()
    h.close()
