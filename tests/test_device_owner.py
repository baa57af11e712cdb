"""slam-eds_amd/csrc/eds_device_owner.hpp, which owns the device and pinned memory, the uploads and the read-backs of eds_imm, eds_ct,
eds_win and eds_sel, of the eds_act / eds_wsv / eds_wed states beside them, and the memory of the tracker handle eds_trk.

Without a device: the owner on its own (tests/cpp/device_owner_check.cpp under AddressSanitizer and UBSan, a stand-alone program), and
the four creators, whose argument checks stay ahead of the device check.  On the device: the same program built plainly; one image
uploaded dense, with a pitched row stride and from device memory (and, for the calls that take several, with a frame stride larger
than a frame) is stored bit for bit the same; and the paths whose frees the owner took over (pointer exchange, the two regrowing
buffer sets, destroy after each) leave a device on which a new window linearizes as a fresh one did.

Already covered elsewhere and not repeated: device-pitched images against the host restatement in test_coarse_gpu.py,
test_immature_gpu.py, test_select_gpu.py (which also has host-pitched) and test_window_gpu.py; destroy after an exchange of the two
buffer sets in every test of test_winedit_gpu.py."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "device_owner_check.cpp")
capi = importlib.import_module("slam-eds_amd.capi")
MODS = {m: importlib.import_module("slam-eds_amd." + m) for m in ("immature", "coarse", "window", "select")}
# the creator of each image-taking handle, its smallest legal arguments with H != W, and the same with an illegal shape
CREATORS = {"immature": ("eds_imm_create", (8, 9, 1, 1, 1), (7, 9, 1, 1, 1)), "coarse": ("eds_ct_create", (8, 9, 1, 1, 1), (8, 9, 2, 1, 1)),
            "window": ("eds_win_create", (8, 9, 2, 1, 1), (7, 9, 2, 1, 1)), "select": ("eds_sel_create", (32, 33), (31, 33))}
DESTROYERS = {"immature": "eds_imm_destroy", "coarse": "eds_ct_destroy", "window": "eds_win_destroy", "select": "eds_sel_destroy"}


def _build(exe, extra=()):
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", *extra, SRC, "-o", str(exe),
                           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"])
    return str(exe)


def _no_device():
    if capi.device_count() > 0:
        pytest.skip("a GPU is visible here; the refusal path is covered on CPU-only hosts")


def test_owner_without_a_device_under_the_sanitizers(tmp_path):
    """open() answers EDS_ERR_NO_DEVICE, alloc() refuses, close() on the owner that never opened is harmless: host code only"""
    _no_device()
    exe = _build(tmp_path / "device_owner_check_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "no device ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("kind", list(CREATORS))
def test_creators_check_their_arguments_before_the_device(capi, kind):
    _no_device()
    name, legal, illegal = CREATORS[kind]
    fn = getattr(MODS[kind]._lib(), name)
    h = C.c_void_p(0xdead)
    assert fn(0, *legal, C.byref(h)) == capi.ERR_NO_DEVICE and not h.value and "no HIP device" in capi.last_error()
    h = C.c_void_p(0xdead)
    assert fn(0, *illegal, C.byref(h)) == capi.ERR_INVALID and not h.value


@pytest.mark.gpu
def test_owner_walk_on_the_device(gpu, tmp_path):
    """open, three buffers, release, a refused 2^60-byte request (alone and in a table), exchanged pointers, a pinned block and a mapped
    pair read through its device pointer, a buffer regrown 256 -> 4096 bytes, refused pinned requests that leave NULL pointers and a zero
    capacity, close twice with both lists empty, reopen"""
    exe = _build(tmp_path / "device_owner_check")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "owner ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _stored(kind, L, h, H, W, frames):
    """the planes the handle stores for its image(s), read back"""
    vp = capi.vp
    if kind == "immature":
        out = np.zeros((2, frames, H, W, 3), np.float32)
        for which in range(2):
            for f in range(frames):
                assert L.eds_imm_get_image(h, which, f, vp(out[which, f])) == 0, capi.last_error()
        return out
    if kind == "coarse":
        out, n = np.zeros((2, H, W, 3), np.float32), C.c_int32()
        for which in range(2):                                   # REF_IMAGE, NEW_IMAGE at level 0
            assert L.eds_ct_get_level(h, which, 0, vp(out[which]), C.cast(C.byref(n), C.c_void_p)) == 0, capi.last_error()
        return out
    if kind == "window":
        out = np.zeros((frames, H, W, 3), np.float32)
        for f in range(frames):
            assert L.eds_win_get_frame(h, f, vp(out[f])) == 0, capi.last_error()
        return out
    out = [np.zeros((H >> l, W >> l, 4), np.float32) for l in range(3)]
    for l in range(3):
        assert L.eds_sel_get_level(h, l, vp(out[l])) == 0, capi.last_error()
    return np.concatenate([o.ravel() for o in out])


def _upload(kind, L, h, ptr, count, fs, rs, dev):
    if kind == "immature":
        rcs = [L.eds_imm_set_host_images(h, 0, count, ptr, fs, rs, dev), L.eds_imm_set_target_images(h, 0, count, ptr, fs, rs, dev)]
    elif kind == "coarse":
        rcs = [L.eds_ct_set_calib(h, 10.0, 11.0, 4.5, 4.0), L.eds_ct_set_ref(h, ptr, rs, dev, 1.0, 0.0, 0.0, 0, None, None, None, None),
               L.eds_ct_set_new(h, ptr, rs, dev, 1.0)]
    elif kind == "window":
        rcs = [L.eds_win_set_frames(h, 0, count, ptr, rs, fs, dev)]
    else:
        rcs = [L.eds_sel_set_image(h, ptr, rs, dev, None)]
    assert rcs == [0] * len(rcs), capi.last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(CREATORS))
def test_dense_pitched_and_device_uploads_store_the_same_bits(gpu, kind):
    name, legal, _ = CREATORS[kind]
    L = MODS[kind]._lib()
    H, W = legal[:2]
    frames = 2 if kind in ("immature", "window") else 1          # the calls that take several images
    if kind == "immature":
        legal = (H, W, 2, 1, 2)
    rng = np.random.default_rng(11)
    img = rng.uniform(0.0, 255.0, (frames, H, W)).astype(np.float32)
    rs, fs = W + 3, (H + 2) * (W + 3) + 5                        # a pitched row, and a frame stride larger than a pitched frame
    pitched = np.full(frames * fs, np.float32(np.nan))
    for f in range(frames):
        pitched[f * fs:f * fs + H * rs].reshape(H, rs)[:, :W] = img[f]
    on_dev = capi.DeviceArray.from_numpy(pitched)
    got = []
    for ptr, a_fs, a_rs, dev in ((capi.vp(img), 0, 0, 0), (capi.vp(pitched), fs, rs, 0), (C.c_void_p(on_dev.ptr), fs, rs, 1)):
        h = C.c_void_p()
        assert getattr(L, name)(0, *legal, C.byref(h)) == 0, capi.last_error()
        _upload(kind, L, h, ptr, frames, a_fs if frames > 1 else 0, a_rs, dev)
        got.append(_stored(kind, L, h, H, W, frames))
        getattr(L, DESTROYERS[kind])(h)
    assert np.isfinite(got[0]).all() and got[0].any()
    assert np.array_equal(_bits(got[0]), _bits(got[1])) and np.array_equal(_bits(got[0]), _bits(got[2]))


def _activation(c, max_points):
    """an eds_imm with room for max_points per host that holds activation case c with the map, the selection and the fit made"""
    imm, act = importlib.import_module("slam-eds_amd.immature"), importlib.import_module("slam-eds_amd.activate")
    h = imm.ImmaturePoints(c.H, c.W, c.F, max_points, 4)
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


@pytest.mark.gpu
def test_exchange_regrow_and_destroy_leave_the_device_as_a_fresh_one(gpu):
    """an edit (the two buffer sets exchange their pointers) -> two inserts from a growing eds_imm (the insert's scratch regrows) -> a
    distance map from a growing set of active points (the staging buffers regrow) -> destroy; a window created afterwards linearizes
    bit for bit as one did before any of it"""
    import winedit_cases as wec
    import winsolve_harness as wsh
    window, winsolve, winedit = (importlib.import_module("slam-eds_amd." + m) for m in ("window", "winsolve", "winedit"))
    s = wec.insert_case("w64_f3")
    c, ac = s.win, s.act

    def linearized():
        w, sv = wsh.open_case(s, window.Window, winsolve.WindowSolver, max_points=len(c.host) + 1, max_residuals=len(c.point) + 1)
        energy, counts = w.linearize(c.F, c.precalc, c.th)
        out = dict(w.residuals(), energy=np.float64(energy), counts=np.asarray(counts))
        w.close()
        return out

    fresh = linearized()
    mp = max(1, max(len(x["uv"]) for x in ac.hosts))
    w, sv = wsh.open_case(s, window.Window, winsolve.WindowSolver, max_points=4096, max_residuals=16384)
    ed = winedit.WindowEdit(w, sv)
    wec.prepare_insert(w, sv, s)
    flags = (np.arange(w.n) % 4 == 0).astype(np.int32)
    removed = ed.remove_points(flags)                            # the exchange
    assert removed[0] == int(flags.sum()) and w.n == len(c.host) - removed[0]
    grown = []
    for room in (mp, 3 * mp + 7):                                # the second eds_imm is larger: the insert's scratch regrows
        h, a = _activation(ac, room)
        K = len(a.activated()["host"])
        n = w.n
        assert K > 0 and ed.insert_activated(a)[0] == K and w.n == n + K
        grown.append((h, a))
    h, a = grown[1]
    a.make_distance_map(ac.newest, ac.KRKi1, ac.Kt1, ac.active_host, ac.active)     # the map of the seeds alone (select has drawn into the last one)
    before = a.distance_map().copy()
    order = np.argsort(np.concatenate([ac.active_host, ac.active_host]), kind="stable")
    a.make_distance_map(ac.newest, ac.KRKi1, ac.Kt1, np.concatenate([ac.active_host, ac.active_host])[order],
                        np.concatenate([ac.active, ac.active])[order])          # twice the active points, from host memory: the staging regrows
    assert len(ac.active_host) > 0 and np.array_equal(a.distance_map(), before)    # every point twice seeds the same map
    w.linearize(c.F, c.precalc, c.th)                            # the exchanged, grown tables are in use
    w.close()
    for h, _ in grown:
        h.close()
    again = linearized()
    assert fresh.keys() == again.keys() and all(wsh.same_bits(fresh[k], again[k]) for k in fresh)
