"""include/eds_hip_immature.h on the device against the numpy oracle (tests/np_immature_oracle.py), bit for bit (any NaN equal to any
NaN): the stored images, the constructors' outputs, and every field after every trace of every sequence of tests/immature_cases.py;
a batch against its singles, host-pointer against device-pointer images, a run against its repetition, and the error codes, each of
which leaves the state as it was."""
import importlib

import numpy as np
import pytest

import immature_cases as ic
import np_immature_oracle as no

pytestmark = pytest.mark.gpu
NAMES = list(ic.cases())
# the oracle's field -> the accessor's
GET = dict(idepth_min="idepth_min", idepth_max="idepth_max", quality="quality", status="lastTraceStatus", last_uv="lastTraceUV",
           last_interval="lastTracePixelInterval")


@pytest.fixture(scope="module")
def imm(capi, gpu):
    return importlib.import_module("slam-eds_amd.immature")


def _open(imm, c, device_images=False, capi=None):
    h = imm.ImmaturePoints(c.H, c.W, len(c.hosts), max(len(x["uv"]) for x in c.hosts), len(c.targets), **c.prm)
    hosts, targets = np.stack([x["image"] for x in c.hosts]), np.stack(c.targets)
    if device_images:
        hosts, targets = capi.DeviceArray.from_numpy(hosts), capi.DeviceArray.from_numpy(targets)
    h.set_host_images(0, hosts)
    h.set_target_images(0, targets)
    alive = [h.create_points(i, x["uv"], x["type"], x["idepth"], x["distance"]) for i, x in enumerate(c.hosts)]
    return h, alive


def _step_args(step):
    return (np.stack([s[0] for s in step]), np.stack([s[1] for s in step]), np.stack([s[2] for s in step]))


def _state(h, n_hosts):
    return [dict(h.get(i), **h.points(i)) for i in range(n_hosts)]


def _same_state(a, b):
    return all(no.same_bits(x[k], y[k]).all() for x, y in zip(a, b) for k in x)


@pytest.mark.parametrize("name", NAMES)
def test_images_points_and_every_trace_equal_the_oracle(imm, name):
    c, o = ic.cases()[name], ic.oracle_run(name)
    h, alive = _open(imm, c)
    for i, ref in enumerate(o["host_images"]):
        assert no.same_bits(h.image(imm.HOST_IMAGE, i), ref).all()
    for k, ref in enumerate(o["target_images"]):
        assert no.same_bits(h.image(imm.TARGET_IMAGE, k), ref).all()
    for i, ref in enumerate(o["after"][0]):
        live, got = ref["alive"], h.points(i)
        assert np.array_equal(alive[i], live) and np.array_equal(got["alive"], live)
        assert np.isnan(got["energyTH"][~live]).all()
        for f in ("color", "weights", "energyTH"):
            assert no.same_bits(got[f][live], ref[f][live]).all(), f
        assert no.same_bits(got["gradH"].reshape(-1, 4)[live], ref["gradH"][live]).all()
    for k, step in enumerate(c.steps):
        summary = h.trace(0, [k] * len(step), *_step_args(step))          # traceNewCoarse: every host against the new frame
        assert np.array_equal(summary, o["summaries"][k]), (name, k)
        for i, ref in enumerate(o["after"][k + 1]):
            got = h.get(i)
            for f, g in GET.items():
                bad = ~no.same_bits(got[g], ref[f])
                assert not bad.any(), (name, k, i, f, np.argwhere(bad)[:5].tolist())
    h.close()


def test_batch_equals_singles_and_device_images_equal_host_images(imm, capi):
    c = ic.cases()["y7_gn3_seeded"]
    hb, _ = _open(imm, c)
    hs, _ = _open(imm, c, device_images=True, capi=capi)
    n = len(c.hosts)
    for k, step in enumerate(c.steps):
        K, t, a = _step_args(step)
        sb = hb.trace(0, [k] * n, K, t, a)
        ss = np.concatenate([hs.trace(i, [k], K[i], t[i], a[i]) for i in (3, 0, 6, 1, 5, 2, 4)])[np.argsort([3, 0, 6, 1, 5, 2, 4])]
        assert np.array_equal(sb, ss)
    assert _same_state(_state(hb, n), _state(hs, n))
    for i in range(n):
        assert no.same_bits(hb.image(imm.HOST_IMAGE, i), hs.image(imm.HOST_IMAGE, i)).all()
    # distinct targets in one call: hosts 0 .. 3 against targets 3, 2, 1, 0 — equal to four single calls
    K, t, a = _step_args(c.steps[0])
    hb.trace(0, [3, 2, 1, 0], K[:4], t[:4], a[:4])
    for i in range(4):
        hs.trace(i, [3 - i], K[i], t[i], a[i])
    assert _same_state(_state(hb, n), _state(hs, n))
    hb.close()
    hs.close()


def test_strided_device_images(imm, capi):
    c = ic.cases()["d1_gn0"]
    pad = np.full((2, c.H + 3, c.W + 5), 7.0, np.float32)
    pad[0, :c.H, :c.W], pad[1, :c.H, :c.W] = c.hosts[0]["image"], c.targets[0]
    d = capi.DeviceArray.from_numpy(pad)
    h = imm.ImmaturePoints(c.H, c.W, 1, 64, 1)
    row = 4 * (c.W + 5)
    h.set_host_images(0, d.view((1, c.H, c.W), (row * (c.H + 3), row, 4)))
    h.set_target_images(0, d.view((1, c.H, c.W), (row * (c.H + 3), row, 4), offset=row * (c.H + 3)))
    o = ic.oracle_run("d1_gn0")
    assert no.same_bits(h.image(imm.HOST_IMAGE, 0), o["host_images"][0]).all()
    assert no.same_bits(h.image(imm.TARGET_IMAGE, 0), o["target_images"][0]).all()
    h.close()


def test_a_run_repeats_exactly(imm):
    c = ic.cases()["x3_gn3"]
    runs = []
    for _ in range(2):
        h, _ = _open(imm, c)
        sums = [h.trace(0, [k] * len(step), *_step_args(step)) for k, step in enumerate(c.steps)]
        runs.append((sums, _state(h, len(c.hosts))))
        h.close()
    assert all(np.array_equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    assert _same_state(runs[0][1], runs[1][1])


def test_error_codes_leave_the_state_unchanged(imm, capi):
    c = ic.cases()["x3_gn3"]
    h, _ = _open(imm, c)
    n = len(c.hosts)
    K, t, a = _step_args(c.steps[0])
    h.trace(0, [0] * n, K, t, a)
    before = _state(h, n)
    images = [h.image(imm.HOST_IMAGE, 0), h.image(imm.TARGET_IMAGE, 1)]

    def refused(code, fn, *args, **kw):
        with pytest.raises(capi.EdsError) as e:
            fn(*args, **kw)
        assert e.value.code == code, e.value
        assert _same_state(before, _state(h, n))
        assert no.same_bits(images[0], h.image(imm.HOST_IMAGE, 0)).all() and no.same_bits(images[1], h.image(imm.TARGET_IMAGE, 1)).all()

    host_mem = np.ascontiguousarray(c.targets[0])
    as_device = (int(host_mem.ctypes.data), host_mem.shape, None, np.float32)       # a host pointer handed over as device memory
    refused(capi.ERR_INVALID, h.set_target_images, 1, as_device)
    refused(capi.ERR_INVALID, h.set_host_images, 0, as_device)
    d = capi.DeviceArray.from_numpy(host_mem)                                        # a device range that runs past its allocation
    refused(capi.ERR_INVALID, h.set_target_images, 0, (d.ptr, (4,) + host_mem.shape, None, np.float32))
    refused(capi.ERR_INVALID, h.trace, 0, [0, len(c.targets), 0], K, t, a)           # target index out of range
    refused(capi.ERR_INVALID, h.trace, 0, [-1] * n, K, t, a)
    for bad in (np.nan, np.inf):
        Kb = K.copy()
        Kb[1, 2, 0] = bad
        refused(capi.ERR_INVALID, h.trace, 0, [0] * n, Kb, t, a)                     # non-finite KRKi
    tb = t.copy()
    tb[2, 1] = np.nan
    refused(capi.ERR_INVALID, h.trace, 0, [0] * n, K, tb, a)
    refused(capi.ERR_INVALID, h.trace, 1, [0] * n, K, t, a)                          # hosts 1 .. 3 of 3
    too_many = np.tile(c.hosts[0]["uv"], (2, 1))[:h.max_points + 1]
    refused(capi.ERR_INVALID, h.create_points, 1, too_many)                          # more points than capacity
    refused(capi.ERR_INVALID, h.create_points, n, c.hosts[0]["uv"])
    refused(capi.ERR_INVALID, h.set_params, trace_gn_iterations=17)
    refused(capi.ERR_INVALID, h.set_params, trace_stepsize=0.0)
    refused(capi.ERR_INVALID, h.set_params, huber_th=float("nan"))
    # ... and the handle still works: the next trace equals the oracle's
    K, t, a = _step_args(c.steps[1])
    assert np.array_equal(h.trace(0, [1] * n, K, t, a), ic.oracle_run("x3_gn3")["summaries"][1])
    h.close()
    # a frame never set, a host without image
    h = imm.ImmaturePoints(c.H, c.W, 1, 8, 2)
    with pytest.raises(capi.EdsError) as e:
        h.create_points(0, c.hosts[0]["uv"][:4])
    assert e.value.code == capi.ERR_STATE
    h.set_host_images(0, c.hosts[0]["image"])
    h.set_target_images(0, c.targets[0])
    h.create_points(0, c.hosts[0]["uv"][8:12])
    with pytest.raises(capi.EdsError) as e:
        h.trace(0, [1], K[0], t[0], a[0])
    assert e.value.code == capi.ERR_STATE
    h.close()
