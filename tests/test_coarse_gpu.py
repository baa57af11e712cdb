"""include/eds_hip_coarse.h on the device against csrc/eds_coarse.hpp under g++ (tests/coarse_harness.py), BIT FOR BIT (any NaN equal to
any NaN) on every case of tests/coarse_cases.py and every output of eds_ct_get_level, eds_ct_calc_res and eds_ct_track; a batch against
its singles, a run against its repetition, device-pointer against host-pointer images, the error codes, and level 0 of the pyramid
against eds_imm_get_image of the same frame."""
import importlib

import numpy as np
import pytest

import coarse_cases as cc
import coarse_harness as ch

pytestmark = pytest.mark.gpu
NAMES = list(cc.cases())


@pytest.fixture(scope="module")
def coarse(capi, gpu):
    return importlib.import_module("slam-eds_amd.coarse")


def same_bits(a, b):
    """bit equality of two arrays or records, any NaN equal to any NaN"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype.names:
        return a.shape == b.shape and all(same_bits(a[k], b[k]) for k in a.dtype.names)
    if a.shape != b.shape:
        return False
    if a.dtype.kind == "f":
        ia, ib = a.view(f"u{a.dtype.itemsize}"), b.view(f"u{a.dtype.itemsize}")
        return bool(((ia == ib) | (np.isnan(a) & np.isnan(b))).all())
    return bool((a == b).all())


def _device(coarse, c, **kw):
    return ch.open_case(c, cls=lambda H, W, levels: coarse.CoarseTracker(H, W, levels, max_points=4096, max_tries=8), **kw)


@pytest.fixture(scope="module")
def host():
    """every case under g++, made once"""
    out = {}
    for name, c in cc.cases().items():
        t = ch.open_case(c)
        out[name] = dict(pc_n=t.pc_n.copy(), K=[t.K(l) for l in range(c.levels)],
                         levels=[[t.level(w, l) for w in range(5)] for l in range(c.levels)],
                         calc=[[t.calc_res(l, T, a) for l in range(c.levels)] for T, a in zip(c.T_init, c.aff_init)],
                         calc_wide=t.calc_res(0, c.T_init[0], c.aff_init[0], cutoff=160.0),
                         track=t.track(c.T_init, c.aff_init, c.coarsest, c.min_res))
        t.close()
    return out


@pytest.mark.parametrize("name", NAMES)
def test_every_output_equals_the_host_restatement_bit_for_bit(coarse, host, name):
    c, h = cc.cases()[name], host[name]
    t = _device(coarse, c)
    assert np.array_equal(t.pc_n, h["pc_n"])
    for l in range(c.levels):
        assert same_bits(t.K(l), h["K"][l])
        for w in range(5):
            assert same_bits(t.level(w, l), h["levels"][l][w]), (name, l, w)
    for k, (T, a) in enumerate(zip(c.T_init, c.aff_init)):
        for l in range(c.levels):
            got, want = t.calc_res(l, T, a), h["calc"][k][l]
            for f in ("rows", "rs", "H", "b"):
                assert same_bits(got[f], want[f]), (name, k, l, f)
    got = t.calc_res(0, c.T_init[0], c.aff_init[0], cutoff=160.0)
    assert all(same_bits(got[f], h["calc_wide"][f]) for f in ("rows", "rs", "H", "b"))
    r = t.track(c.T_init, c.aff_init, c.coarsest, c.min_res)
    for f in r.dtype.names:
        assert same_bits(r[f], h["track"][f]), (name, f, r[f], h["track"][f])
    t.close()


def test_a_batch_of_8_equals_its_singles_and_a_run_repeats(coarse):
    c = cc.cases()["b96_l4"]
    rng = np.random.default_rng(11)
    tries = np.stack([cc.se3(0.01 * rng.standard_normal(3), 0.02 * rng.standard_normal(3)) for _ in range(8)])
    affs = np.stack([0.02 * rng.standard_normal(8), 3.0 * rng.standard_normal(8)], axis=1)
    t = _device(coarse, c)
    batch = t.track(tries, affs, c.coarsest, c.min_res)
    singles = np.concatenate([t.track(tries[k], affs[k], c.coarsest, c.min_res) for k in (5, 0, 7, 2, 1, 6, 3, 4)])[np.argsort([5, 0, 7, 2, 1, 6, 3, 4])]
    assert same_bits(batch, singles)
    assert batch["ok"].sum() >= 6 and len({r.tobytes() for r in batch["T"]}) == 8
    t.close()
    t2 = _device(coarse, c)
    assert same_bits(t2.track(tries, affs, c.coarsest, c.min_res), batch)
    t2.close()


def test_device_pointer_images_equal_host_images_and_wrong_pointers_are_refused(coarse, capi, host):
    c = cc.cases()["a64_l3"]
    pad = np.full((2, c.H + 3, c.W + 5), 7.0, np.float32)
    pad[0, :c.H, :c.W], pad[1, :c.H, :c.W] = c.ref, c.new
    d = capi.DeviceArray.from_numpy(pad)
    row = 4 * (c.W + 5)
    t = coarse.CoarseTracker(c.H, c.W, c.levels, max_points=4096, max_tries=8)
    t.set_params(**c.prm)
    t.set_calib(*c.K)
    pc_n, dropped = t.set_ref(d.view((c.H, c.W), (row, 4)), c.cp, c.hdif, c.exposure_ref, c.aff_ref)
    t.set_new(d.view((c.H, c.W), (row, 4), offset=row * (c.H + 3)), c.exposure_new)
    assert np.array_equal(pc_n, host["a64_l3"]["pc_n"]) and dropped >= 3
    for l in range(c.levels):
        for w in range(5):
            assert same_bits(t.level(w, l), host["a64_l3"]["levels"][l][w])
    before = t.track(c.T_init, c.aff_init, c.coarsest, c.min_res)
    assert same_bits(before, host["a64_l3"]["track"])

    def refused(code, fn, *args, **kw):
        with pytest.raises(capi.EdsError) as e:
            fn(*args, **kw)
        assert e.value.code == code, e.value

    host_mem = np.ascontiguousarray(c.new)
    as_device = (int(host_mem.ctypes.data), host_mem.shape, None, np.float32)          # a host pointer handed over as device memory
    refused(capi.ERR_INVALID, t.set_new, as_device)
    refused(capi.ERR_INVALID, t.set_ref, as_device, c.cp, c.hdif)
    small = capi.DeviceArray.from_numpy(host_mem[:8])                                  # a device range that runs past its allocation
    refused(capi.ERR_INVALID, t.set_new, (small.ptr, host_mem.shape, None, np.float32))
    refused(capi.ERR_INVALID, t.track, np.full((1, 3, 4), np.nan))
    refused(capi.ERR_INVALID, t.track, c.T_init[0], [[np.inf, 0.0]])
    refused(capi.ERR_INVALID, t.track, c.T_init[0], None, c.levels)
    refused(capi.ERR_INVALID, t.track, np.tile(c.T_init[0], (9, 1, 1)))
    refused(capi.ERR_INVALID, t.set_params, huber_th=0.0)
    refused(capi.ERR_INVALID, t.set_params, coarse_cutoff_th=float("nan"))
    refused(capi.ERR_INVALID, t.set_calib, 0.0, 50.0, 1.0, 1.0)
    refused(capi.ERR_INVALID, t.set_ref, c.ref, np.zeros((4097, 3)), np.ones(4097))
    # every refusal left the state as it was
    assert same_bits(t.track(c.T_init, c.aff_init, c.coarsest, c.min_res), before)
    t.close()
    for bad in ((48, 64, 4), (50, 64, 3), (48, 64, 6), (48, 64, 3, coarse.MAX_POINTS + 1), (48, 64, 3, 100, 0)):
        with pytest.raises(capi.EdsError) as e:
            coarse.CoarseTracker(*bad)
        assert e.value.code == capi.ERR_INVALID
    t = coarse.CoarseTracker(c.H, c.W, c.levels)
    refused(capi.ERR_STATE, t.set_ref, c.ref, c.cp, c.hdif)                            # no calibration yet
    t.set_calib(*c.K)
    refused(capi.ERR_STATE, t.track, c.T_init[0])                                      # no frames yet
    t.set_ref(c.ref, c.cp, c.hdif)
    refused(capi.ERR_STATE, t.track, c.T_init[0])                                      # no new frame yet
    refused(capi.ERR_STATE, t.level, coarse.NEW_IMAGE, 0)
    t.close()


def test_level_0_equals_the_immature_trace_images(coarse):
    imm = importlib.import_module("slam-eds_amd.immature")
    c = cc.cases()["b96_l4"]
    t = _device(coarse, c)
    h = imm.ImmaturePoints(c.H, c.W, 1, 8, 1)
    h.set_host_images(0, c.ref)
    h.set_target_images(0, c.new)
    assert same_bits(t.level(coarse.REF_IMAGE, 0), h.image(imm.HOST_IMAGE, 0))
    assert same_bits(t.level(coarse.NEW_IMAGE, 0), h.image(imm.TARGET_IMAGE, 0))
    h.close()
    t.close()


def test_the_scatter_at_its_worst_case_equals_the_serial_loop(coarse):
    """EDS_CT_MAX_POINTS contributions, two per pixel, the second a whole half of the inputs after the first: every colliding pixel's
    walk is as long as it can be and there are as many of them as there can be.  idepth and weightSums equal the serial loop's."""
    import time
    n, H, W = coarse.MAX_POINTS, 256, 256
    rng = np.random.default_rng(3)
    pix = np.tile(rng.permutation(H * W)[:n // 2], 2)
    cp = np.stack([pix % W + rng.uniform(-0.4, 0.4, n), pix // W + rng.uniform(-0.4, 0.4, n), rng.uniform(0.1, 2.0, n)], axis=1).astype(np.float32)
    hdif = rng.uniform(0.5, 400.0, n).astype(np.float32)
    img = cc.texture(*np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))).astype(np.float32)
    t, h = coarse.CoarseTracker(H, W, 2, max_points=n, max_tries=1), ch.HostTracker(H, W, 2)
    for x in (t, h):
        x.set_calib(200.0, 210.0, 127.0, 126.0)
    t.set_ref(img, cp, hdif)                                     # warm-up
    t0 = time.perf_counter()
    got = t.set_ref(img, cp, hdif)
    dt = time.perf_counter() - t0
    want = h.set_ref(img, cp, hdif)
    print(f"worst-case scatter of {n} contributions: eds_ct_set_ref {dt * 1e3:.2f} ms")
    assert np.array_equal(got[0], want[0]) and got[1] == want[1] == 0
    for l in range(2):
        for which in (coarse.IDEPTH, coarse.WEIGHT_SUMS, coarse.PC):
            assert same_bits(t.level(which, l), h.level(which, l)), (l, which)
    t.close()
    h.close()
