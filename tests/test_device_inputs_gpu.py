"""Inputs that already live in device memory (include/eds_hip_device.h) against the host entry points fed the same values.

Equality is exact everywhere: the device path narrows with the same rule (round-to-nearest-even, fp32 denormals kept, overflow to
+-inf), stores the same tiles and margin, and forms the keyframe planes with the same uncontracted fp64 arithmetic, so a slot filled
either way holds the same bits and every solve on it takes the same steps.  Device buffers come from capi.DeviceArray (the HIP
runtime the library is bound to); torch appears only in one child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 40


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def _special_frames(rng, count, H, W):
    """fp64 frames whose values exercise the narrowing: NaN, +-0, an fp32 denormal, fp32 overflow both ways, ties between two fp32
    neighbours (to even, both directions) — in the corners (the margin replicates them), on the borders and inside"""
    f = rng.standard_normal((count, H, W))
    special = np.array([np.nan, 0.0, -0.0, 1e-40, -1e-40, 1e39, -1e39, 1.0 + 2.0 ** -24, 1.0 + 3.0 * 2.0 ** -24, -(1.0 + 2.0 ** -24),
                        3.4028235677973366e38, 1e-46])
    for b in range(count):
        r = rng.integers(0, H, size=4 * len(special))
        c = rng.integers(0, W, size=4 * len(special))
        f[b, r, c] = np.tile(special, 4)
        k = b % len(special)
        f[b, 0, 0], f[b, 0, W - 1], f[b, H - 1, 0], f[b, H - 1, W - 1] = special[k], special[(k + 3) % 12], special[(k + 5) % 12], special[(k + 7) % 12]
    return f


def _on_device(capi, frames, pitched):
    """the frames as a device array: dense, or rows W + 3 apart and frames H * (W + 3) + 5 apart inside a buffer that ends with the last
    element read (so the extent the library checks is the exact one)"""
    count, H, W = frames.shape
    if not pitched:
        return capi.DeviceArray.from_numpy(frames)
    it = frames.dtype.itemsize
    row, frame = W + 3, H * (W + 3) + 5
    buf = np.full((count - 1) * frame + (H - 1) * row + W, 777.0, dtype=frames.dtype)
    for b in range(count):
        for r in range(H):
            o = b * frame + r * row
            buf[o:o + W] = frames[b, r]
    return capi.DeviceArray.from_numpy(buf).view((count, H, W), (frame * it, row * it, it))


@pytest.mark.parametrize("layout", ["tiles", "rowmajor"])
@pytest.mark.parametrize("H,W", [(40, 52), (37, 50)])
def test_frames_from_device_memory_have_the_host_paths_bits(gpu, capi, monkeypatch, H, W, layout):
    if layout == "rowmajor":
        monkeypatch.setenv("EDS_FRAME_LAYOUT", "rowmajor")      # read at create
    else:
        monkeypatch.delenv("EDS_FRAME_LAYOUT", raising=False)
    cfg = capi.default_config()
    hd, hh = capi.Handle(cfg, B, 64, H, W), capi.Handle(cfg, B, 64, H, W)
    rng = np.random.default_rng(H * 1000 + W)
    first = 2
    for dtype in (np.float32, np.float64):
        for pitched in (False, True):
            for count in (1, 5, 33):
                with np.errstate(over="ignore", under="ignore", invalid="ignore"):
                    frames = np.ascontiguousarray(_special_frames(rng, count, H, W).astype(dtype))
                d = _on_device(capi, frames, pitched)
                hd.set_event_frames_device(first, d)
                hh.set_event_frames(first, [frames[b] for b in range(count)])
                for s in range(B):          # the slots of the range, and nobody else's
                    got, ref = hd.get_event_frame(s), hh.get_event_frame(s)
                    assert _same(got, ref), (dtype.__name__, pitched, count, s)
                with np.errstate(over="ignore", under="ignore", invalid="ignore"):
                    want = frames[count - 1].astype(np.float32).astype(np.float64)
                assert _same(hd.get_event_frame(first + count - 1), want)
                hd.sync()                   # the source is freed below: the kernel that read it has finished
                del d
    hd.close(); hh.close()


def _border_alignments(synth):
    """four alignments on 64 x 48, N = 64 .. 200; some points moved to within 2 px of each border, a few outside the frame"""
    als = []
    for k, n in enumerate((64, 100, 150, 200)):
        al = synth.make_alignment(300 + k, H=48, W=64, N=n)
        px = np.array([0.5, 62.4, 20.25, 31.5, 1.75, 63.0, -3.0, 30.0, 66.5])
        py = np.array([10.0, 20.5, 0.7, 46.6, 1.2, 47.0, 12.0, 50.5, -1.5])
        idx = np.arange(len(px)) * (n // len(px))
        al.norm_coord[idx, 0] = (px - al.cx) / al.fx
        al.norm_coord[idx, 1] = (py - al.cy) / al.fy
        als.append(al)
    return als


def _residual_bits(capi, h, b):
    try:
        return _bits(h.residuals(b))
    except capi.EdsError as e:
        return e.code


REF12_SPREAD = 1e-9      # the bound tests/test_groups_gpu.py holds REF12's persistent kernel to against itself


def _solve_and_compare(capi, hd, hh, als, first=0, exact=None):
    """one batched solve on each handle from the alignments' start states; results table (poses, velocities, costs, iteration counts,
    success), residual vectors and info compared bit for bit.  exact[b] = False: slot b's floating-point outcomes are compared to
    REF12_SPREAD instead (see test_solves_on_device_fed_frames_are_bit_identical); its counts and flags stay exact."""
    exact = [True] * len(als) if exact is None else exact
    for h in (hd, hh):
        h.set_states(first, [a.p0 for a in als], [a.q0 for a in als], [a.v0 for a in als])
        h.optimize_batch(0, first, len(als))
    rd, rh = hd.results(first, len(als)), hh.results(first, len(als))
    near = lambda a, b: np.all(np.abs(np.asarray(a) - np.asarray(b)) <= REF12_SPREAD * (1.0 + np.abs(np.asarray(b))))
    for j, b in enumerate(range(first, first + len(als))):
        resd, resh = _residual_bits(capi, hd, b), _residual_bits(capi, hh, b)
        id_, ih = hd.info(b), hh.info(b)
        assert _same(rd[j, 14:], rh[j, 14:]), (b, rd[j, 14:], rh[j, 14:])          # iteration count, success
        for k in ("num_points", "num_iterations", "success", "termination"):
            assert id_[k] == ih[k], (b, k)
        if exact[j]:
            assert _same(rd[j], rh[j]), (b, np.abs(rd[j] - rh[j]).max())
            assert np.array_equal(resd, resh), b
            for k in ("initial_cost", "final_cost"):
                assert _same(np.float64(id_[k]), np.float64(ih[k])), (b, k)
        else:
            assert near(rd[j], rh[j]), (b, np.abs(rd[j] - rh[j]).max())
            assert near(hd.residuals(b), hh.residuals(b)), b
            assert near([id_["initial_cost"], id_["final_cost"]], [ih["initial_cost"], ih["final_cost"]]), b
    return rd


@pytest.mark.parametrize("solver", ["LM6", "REF12"])
def test_solves_on_device_fed_frames_are_bit_identical(gpu, capi, synth, solver):
    """Four alignments (N = 64, 100, 150, 200 on 64 x 48, points near every border and outside), frames handed over through the device
    path on one handle and through eds_trk_set_event_frames on its twin, exec = device: results, iteration counts and residual vectors
    are bit-identical.  Solved twice so that the strip copies exist, then other frames through the device path and solved again — the
    case a missed frame_version bump breaks.

    REF12's persistent kernel is not bit-reproducible against ITSELF above 128 points: its wavefronts add their 64-point tiles into
    the LDS sums with fp64 atomics, so with three or more tiles per sum the order, and with it the last bits, vary from run to run
    (tests/test_launch_info_gpu.py, test_groups_gpu.py and test_completion_words_gpu.py say the same).  Measured with this test's
    inputs on MI355X, three rounds: two handles fed the SAME host frames differ in the N = 150 and N = 200 rows by up to 9.3e-15
    (poses, velocities, cost), a device-fed and a host-fed one by up to 2.1e-14; the N = 64 and N = 100 rows (one or two tiles per sum:
    a + b = b + a) never differ, and neither does any iteration count.  So for REF12 the persistent kernel is held to bit-identity on
    the two order-free alignments and to REF12_SPREAD on the other two, and all four are solved once more with EDS_REF12_EXEC=host
    (the host-driven LM loop over the streaming residual / Jacobian / reduction kernels, which sample the same frames in HBM and sum in
    a fixed order), where bit-identity holds for every alignment.  LM6 is bit-identical throughout."""
    als = _border_alignments(synth)
    ref12 = solver == "REF12"
    exact = [a.N <= 128 for a in als] if ref12 else None
    cfg = capi.default_config(solver=getattr(capi, "SOLVER_" + solver), exec=capi.EXEC_DEVICE, max_num_iterations=6)
    hd, hh = capi.Handle(cfg, 4, 200, 48, 64), capi.Handle(cfg, 4, 200, 48, 64)
    for b, a in enumerate(als):
        for h in (hd, hh):
            h.set_keyframe(b, a.norm_coord, a.grad, a.idp, a.weights, a.fx, a.fy, a.cx, a.cy)
    frames = np.stack([a.frame for a in als])
    d = capi.DeviceArray.from_numpy(frames)
    hd.set_event_frames_device(0, d)
    hh.set_event_frames(0, list(frames))
    for s in range(4):
        assert _same(hd.get_event_frame(s), hh.get_event_frame(s))
    r1 = _solve_and_compare(capi, hd, hh, als, exact=exact)
    r2 = _solve_and_compare(capi, hd, hh, als, exact=exact)        # solved again: the strip copies exist now
    assert _same(r1, r2) or ref12
    assert np.all(r1[:, 14] >= 1)                                   # the solver did iterate
    # other frames through the device path: a strip copy made for the earlier ones must be remade (frame_version)
    frames2 = np.ascontiguousarray(frames[[1, 2, 3, 0]] * -1.25)
    d2 = capi.DeviceArray.from_numpy(frames2.astype(np.float32))
    hd.set_event_frames_device(0, d2)
    hh.set_event_frames(0, list(frames2.astype(np.float32)))
    r3 = _solve_and_compare(capi, hd, hh, als, exact=exact)
    assert not _same(r3, r1)
    if ref12:                                                       # the same arithmetic in a fixed order: every alignment, bit for bit
        for h in (hd, hh):
            h.set_knob("EDS_REF12_EXEC", "host")
        r4 = _solve_and_compare(capi, hd, hh, als)
        assert np.all(r4[:, 14] >= 1)
        hd.set_event_frames_device(0, d)
        hh.set_event_frames(0, list(frames))
        _solve_and_compare(capi, hd, hh, als)
    hd.sync(); hh.sync()
    hd.close(); hh.close()


def test_device_ingest_ends_frame_sharing(gpu, capi):
    H, W = 40, 52
    h = capi.Handle(capi.default_config(), 4, 64, H, W)
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal((H, W)), rng.standard_normal((H, W))
    f32 = lambda x: x.astype(np.float32).astype(np.float64)
    h.set_event_frame(1, a)
    h.share_event_frame(3, 1)
    assert _same(h.get_event_frame(3), f32(a))
    d = capi.DeviceArray.from_numpy(b)
    h.set_event_frames_device(3, d)                         # H x W: one frame
    assert _same(h.get_event_frame(3), f32(b))
    assert _same(h.get_event_frame(1), f32(a))
    h.set_event_frame(1, -a)                                # ... and slot 3 no longer follows slot 1
    assert _same(h.get_event_frame(3), f32(b))
    h.close()


@pytest.mark.parametrize("use_exp", [True, False])
def test_event_slices_from_device_memory(gpu, capi, use_exp):
    """Three slices of 0, 1 and 1 000 events.  The vote adds with fp64 atomics, so a pixel's sum depends on the order of its adds
    whenever two events of a slice land on it with inexact terms — on either path.  Two cases in which the order cannot matter, so
    that exact equality is owed: window weights with every event of a slice on a pixel of its own (one add per pixel), and unit
    weights with colliding events (sums of +-1 are exact).  No undistortion map: an event votes for its own pixel only.  The sums of
    squares are one add per accumulator at this frame height (H / 4 workgroups <= 64 accumulators)."""
    H, W = 40, 52
    rng = np.random.default_rng(11)
    if use_exp:
        flat = rng.choice(H * W, size=1000, replace=False)
    else:
        flat = rng.integers(0, H * W // 4, size=1000)
    big = ((flat % W).astype(np.uint16), (flat // W).astype(np.uint16), rng.integers(0, 2, size=1000).astype(np.uint8))
    one = (np.array([W - 1], np.uint16), np.array([H - 1], np.uint16), np.array([1], np.uint8))
    none = (np.zeros(0, np.uint16), np.zeros(0, np.uint16), np.zeros(0, np.uint8))
    slices = [none, one, big]
    cfg = capi.default_config()
    hd, hh = capi.Handle(cfg, 4, 64, H, W), capi.Handle(cfg, 4, 64, H, W)
    ref = hh.build_event_frame_batch(1, slices, use_exp_weights=use_exp)
    offs = np.cumsum([0] + [len(s[0]) for s in slices])
    dx, dy, dp = (capi.DeviceArray.from_numpy(np.concatenate([s[k] for s in slices])) for k in range(3))
    got = hd.build_event_frames_device(1, offs, dx, dy, dp, use_exp_weights=use_exp)
    assert _same(got, ref) and ref[0] == 0.0 and ref[1] > 0.0 and ref[2] > 0.0
    for s in range(4):
        assert _same(hd.get_event_frame(s), hh.get_event_frame(s)), s
    assert np.count_nonzero(hh.get_event_frame(3)) > 300
    # count = 1, the single-slice case, from an offset into the arrays
    ref1 = hh.build_event_frame_batch(0, [big], use_exp_weights=use_exp)
    got1 = hd.build_event_frames_device(0, offs[2:], dx, dy, dp, use_exp_weights=use_exp)
    assert _same(got1, ref1) and _same(hd.get_event_frame(0), hh.get_event_frame(0))
    hd.close(); hh.close()


def _codes(capi, h, calls):
    out = []
    for fn in calls:
        try:
            fn(h)
            out.append(capi.EDS_OK)
        except capi.EdsError as e:
            out.append(e.code)
    return out


def test_keyframes_from_device_memory(gpu, capi, synth):
    H, W, MAXP = 48, 64, 300
    first, Ns, stride = 1, (1, 65, MAXP), MAXP + 7
    cfg = capi.default_config(solver=capi.SOLVER_LM6, exec=capi.EXEC_DEVICE, max_num_iterations=5)
    hd, hh = capi.Handle(cfg, 5, MAXP, H, W), capi.Handle(cfg, 5, MAXP, H, W)
    als = [synth.make_alignment(410 + k, H=H, W=W, N=n) for k, n in enumerate(Ns)]
    frames = [a.frame for a in als]
    # state that a new keyframe must drop: seeds of the depth filter and epiline correspondences, on sane keyframes first
    sane = [synth.make_alignment(420 + k, H=H, W=W, N=64) for k in range(3)]
    pack = lambda rows: np.ascontiguousarray(np.stack([np.concatenate([r, np.full((stride - len(r),) + r.shape[1:], 9e9)]) for r in rows]))
    dev = lambda als_: [capi.DeviceArray.from_numpy(pack([getattr(a, n) for a in als_])) for n in
                        ("norm_coord", "grad", "idp", "weights")]
    Ksane = np.array([[a.fx, a.fy, a.cx, a.cy] for a in sane])
    sane_arrays = dev(sane)
    hd.set_keyframes_device(first, [a.N for a in sane], *sane_arrays, Ksane)
    for b, a in enumerate(sane):
        hh.set_keyframe(first + b, a.norm_coord, a.grad, a.idp, a.weights, a.fx, a.fy, a.cx, a.cy)
    stateful = [lambda h: h.depth_get(first + 1), lambda h: h.epi_get(first + 1), lambda h: h.depth_update(first, 3)]
    for h in (hd, hh):
        h.set_event_frames(first, frames)
        h.set_states(first, [a.p0 for a in sane], [a.q0 for a in sane], [a.v0 for a in sane])
        assert _codes(capi, h, stateful[:2]) == [capi.ERR_STATE] * 2
        h.depth_init(first, 3)
        h.epi_track_points(first, 3, patch_radius=2, erase=False)
        assert _codes(capi, h, stateful[:2]) == [capi.EDS_OK] * 2
    assert _same(hd.epi_get(first + 1), hh.epi_get(first + 1))

    # the keyframes of the test: N = 1, 65 and max_points, a K of its own per slot, u0 / v0 at +-1e6 in the middle one (the clamp)
    K = np.array([[a.fx * (1 + 0.01 * k), a.fy * (1 - 0.02 * k), a.cx + 0.3 * k, a.cy - 0.7 * k] for k, a in enumerate(als)])
    far = als[1]
    far.norm_coord[3] = [(1e6 - K[1, 2]) / K[1, 0], 0.01]
    far.norm_coord[17] = [-0.02, (-1e6 - K[1, 3]) / K[1, 1]]
    far.norm_coord[40] = [(-1e6 - K[1, 2]) / K[1, 0], (1e6 - K[1, 3]) / K[1, 1]]
    far.norm_coord[41] = [(40000.0 - K[1, 2]) / K[1, 0], (-31999.5 - K[1, 3]) / K[1, 1]]
    arrays = dev(als)
    hd.set_keyframes_device(first, list(Ns), *arrays, K)
    for b, a in enumerate(als):
        hh.set_keyframe(first + b, a.norm_coord, a.grad, a.idp, a.weights, *K[b])
    # what needs seeds or correspondences answers as after set_keyframe
    assert _codes(capi, hd, stateful) == _codes(capi, hh, stateful) == [capi.ERR_STATE] * 3
    # the planes, through everything that reads them: residuals, Jacobian, normal equations (eval reads the host's Gram copy) ...
    for b, a in enumerate(als):
        for ncols in (6, 12):
            ed, eh = (h.eval(first + b, a.p_true, a.q_true, a.v0, ncols=ncols) for h in (hd, hh))
            for k in ("r", "J", "JtJ", "Jtr"):
                assert _same(ed[k], eh[k]), (b, ncols, k)
            assert _same(np.float64(ed["cost"]), np.float64(eh["cost"]))
            assert ed["r"].shape == (Ns[b],)
    # ... and a solve on the device (the Gram matrices in HBM)
    _solve_and_compare(capi, hd, hh, als, first)
    hd.sync(); hh.sync()
    hd.close(); hh.close()


def test_idepths_from_device_memory(gpu, capi, synth):
    H, W = 48, 64
    first, Ns = 1, (64, 100, 200)
    cfg = capi.default_config(solver=capi.SOLVER_LM6, exec=capi.EXEC_DEVICE, max_num_iterations=5)
    hd, hh = capi.Handle(cfg, 4, 200, H, W), capi.Handle(cfg, 4, 200, H, W)
    als = [synth.make_alignment(500 + k, H=H, W=W, N=n) for k, n in enumerate(Ns)]
    for h in (hd, hh):
        for b, a in enumerate(als):
            h.set_alignment(first + b, a)
    rng = np.random.default_rng(3)
    S = 207
    # dense rows of doubles
    idp = rng.uniform(0.1, 1.2, size=(3, S))
    idp[0, 5], idp[1, 7], idp[2, 199] = 1e-40, 1e39, 0.0
    d = capi.DeviceArray.from_numpy(idp)
    hd.set_idepths_device(first, d)
    for b, n in enumerate(Ns):
        hh.set_idepth(first + b, idp[b, :n])
    for b, a in enumerate(als):
        ed, eh = (h.eval(first + b, a.p_true, a.q_true, a.v0, ncols=12) for h in (hd, hh))
        assert all(_same(ed[k], eh[k]) for k in ("r", "J", "JtJ", "Jtr"))
    # column 0 of an N x 4 table per slot (what DepthPoints keeps), then a solve on the Gram matrices in HBM
    table = rng.uniform(0.2, 1.0, size=(3, S, 4))
    d4 = capi.DeviceArray.from_numpy(table)
    hd.set_idepths_device(first, d4)
    for b, n in enumerate(Ns):
        hh.set_idepth_strided(first + b, table[b, :n])
    r = _solve_and_compare(capi, hd, hh, als, first)
    assert np.all(r[:, 14] >= 1)
    # a slot without keyframe: the state error of the host call
    with pytest.raises(capi.EdsError) as e:
        hd.set_idepths_device(0, d)
    assert e.value.code == capi.ERR_STATE
    hd.sync(); hh.sync()
    hd.close(); hh.close()


def test_check_range_alone(gpu, capi):
    """no ingest call ever sees one of the bad pointers: eds_dev_check_range launches nothing"""
    host = np.zeros(4096, np.uint8)
    assert capi.check_range(host.ctypes.data, 16) == capi.ERR_INVALID
    assert "pointer" in capi.last_error()
    d = capi.DeviceArray(1000, np.uint8)
    assert capi.check_range(d.ptr, 1000) == capi.EDS_OK
    assert capi.check_range(d.ptr, 1001) == capi.ERR_INVALID and "past its allocation" in capi.last_error()
    assert capi.check_range(d.ptr + 100, 900) == capi.EDS_OK          # an interior pointer with a fitting extent
    assert capi.check_range(d.ptr + 100, 901) == capi.ERR_INVALID
    assert capi.check_range(d.ptr + 999, 1) == capi.EDS_OK
    assert capi.check_range(0, 16) == capi.ERR_INVALID and "NULL" in capi.last_error()
    assert capi.check_range(d.ptr, 2 ** 63) == capi.ERR_INVALID


def test_bad_ranges_return_before_the_pointer_is_looked_at(gpu, capi):
    import ctypes as C
    H, W = 40, 52
    h = capi.Handle(capi.default_config(), 4, 64, H, W)
    d = capi.DeviceArray((4, H, W), np.float32)
    L, p = capi.lib(), C.c_void_p(d.ptr)
    N, K = (C.c_int32 * 4)(1, 1, 1, 1), (C.c_double * 16)(*([1.0] * 16))
    offs = (C.c_int32 * 5)(0, 0, 0, 0, 0)
    for first, count in ((0, 0), (2, 3), (-1, 1), (4, 1)):
        assert L.eds_dev_set_event_frames(h._h, first, count, capi.IMG_F32, p, 0, 0) == capi.ERR_INVALID
        assert "slot range" in capi.last_error()
        assert L.eds_dev_set_keyframes(h._h, first, count, N, p, p, p, p, 64, K) == capi.ERR_INVALID and "slot range" in capi.last_error()
        assert L.eds_dev_set_idepths(h._h, first, count, p, 64, 1) == capi.ERR_INVALID and "slot range" in capi.last_error()
        assert L.eds_dev_build_event_frames(h._h, first, count, offs, p, p, p, 0, 0.5, 1, None) == capi.ERR_INVALID and "slot range" in capi.last_error()
    # the Python layer refuses a shape that does not fit the handle before the library is called
    with pytest.raises(ValueError):
        h.set_event_frames_device(0, capi.DeviceArray((2, H, W + 4), np.float32))
    # and the library refuses what the Python layer cannot know: more frames than slots behind `first`
    with pytest.raises(capi.EdsError) as e:
        h.set_event_frames_device(1, d)
    assert e.value.code == capi.ERR_INVALID
    h.close()


def test_tracker_optimize_takes_a_device_frame(gpu, capi, synth):
    trk = __import__("importlib").import_module("slam-eds_amd.tracker")
    al = synth.make_alignment(77, H=48, W=64, N=150)
    K = np.array([[al.fx, 0, al.cx], [0, al.fy, al.cy], [0, 0, 1.0]])
    out = []
    for device in (True, False):
        kf = trk.KeyFrame(al.norm_coord, al.grad, al.weights, al.idp, K, al.H, al.W)
        t = trk.Tracker(kf, trk.Config(solver=capi.SOLVER_LM6, options=trk.SolverOptions(max_num_iterations=[6])))
        frame = capi.DeviceArray.from_numpy(al.frame) if device else al.frame
        ok, T = t.optimize(0, frame, np.eye(4), px=al.p0, qx=al.q0, vx=al.v0)
        assert ok
        out.append(np.concatenate([t.px, t.qx, t.vx, T.ravel(), kf.residuals]))
        t.close()
    assert _same(out[0], out[1])


_TORCH_CHILD = r"""
import importlib, sys
import numpy as np
import torch                                  # before capi: one process holds one libamdhip64 (capi.torch_loaded_first)
sys.path.insert(0, sys.argv[1])
capi = importlib.import_module("slam-eds_amd.capi")
synth = importlib.import_module("slam-eds_amd.synth")
capi.build()
al = synth.make_alignment(88, H=48, W=64, N=150)
cfg = capi.default_config(solver=capi.SOLVER_LM6, exec=capi.EXEC_DEVICE, max_num_iterations=6)
hd, hh = capi.Handle(cfg, 1, 150, 48, 64), capi.Handle(cfg, 1, 150, 48, 64)
assert capi.torch_loaded_first
side = torch.cuda.Stream()
src = torch.from_numpy(al.frame).to("cuda")
torch.cuda.synchronize()
with torch.cuda.stream(side):                 # the frame is made by torch kernels on a side stream
    t = (src.float() * 0.5 + src.float() * 0.5).contiguous()
hd.wait_stream(side)
hd.set_event_frames_device(0, t)
hd.signal_stream(side)                        # torch may reuse t's memory behind this
host = t.cpu().numpy()
assert host.dtype == np.float32 and host.shape == (48, 64)
hh.set_event_frame(0, host)
res = []
for h in (hd, hh):
    h.set_keyframe(0, al.norm_coord, al.grad, al.idp, al.weights, al.fx, al.fy, al.cx, al.cy)
    p, q, v, info = h.optimize(0, p=al.p0, q=al.q0, v=al.v0)
    res.append(np.concatenate([p, q, v, [info["final_cost"], info["num_iterations"]], h.residuals(0), h.get_event_frame(0).ravel()]))
assert np.array_equal(res[0].view(np.uint64), res[1].view(np.uint64))
# a pitched view of a torch tensor, on the null stream
big = torch.zeros((2, 48, 70), dtype=torch.float64, device="cuda")
big[:, :, :64] = torch.from_numpy(np.stack([al.frame, -al.frame])).to("cuda")
h2a, h2b = capi.Handle(cfg, 2, 150, 48, 64), capi.Handle(cfg, 2, 150, 48, 64)
h2a.wait_stream(torch.cuda.current_stream())
h2a.set_event_frames_device(0, big[:, :, :64])
h2a.signal_stream(torch.cuda.current_stream())
h2b.set_event_frames(0, [al.frame, -al.frame])
for s in range(2):
    assert np.array_equal(h2a.get_event_frame(s).view(np.uint64), h2b.get_event_frame(s).view(np.uint64))
try:
    h2a.set_event_frames_device(0, big.transpose(1, 2)[:, :64, :48])
    raise SystemExit("a transposed view was accepted")
except ValueError:
    pass
print("DEVICE-INPUTS-TORCH-OK")
"""


def test_torch_tensor_on_a_side_stream(gpu, capi):
    """A frame produced by torch on a side stream, handed over with wait_stream -> set_event_frames_device -> signal_stream, solves
    to the host path's bits.  This exercises the ordering calls; it cannot PROVE the ordering (a missing wait usually goes unnoticed
    on a frame this small)."""
    out = subprocess.run([sys.executable, "-c", _TORCH_CHILD, ROOT], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0 and "DEVICE-INPUTS-TORCH-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
