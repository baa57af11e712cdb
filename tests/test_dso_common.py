"""slam-eds_amd/csrc/eds_dso_common.hpp, what the DSO-side kernels and their g++ restatements share.

Without a device: the header under g++ (tests/host_logic/dso_common_harness.cpp) on a 7 x 9 and a 32 x 33 image: make_levels against the
coarse oracle's makeImages, bilin / mix against the window oracle's getInterpolatedElement33, both bit for bit.  On the device:
tests/cpp/dso_common_check.hip, a stand-alone program, once: block_rank<T> in sweeping workgroups of 256, 512 and 1 024 threads, the
two-kernel grid compaction with blocks_before, wave_fold + add8 against reduce_lanes, wave_fold_i."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import harness_build as hb
import header_checks as hc
import np_coarse_oracle as nco
import np_window_oracle as nwo

HERE = os.path.dirname(os.path.abspath(__file__))
capi = importlib.import_module("slam-eds_amd.capi")
SHAPES = [(7, 9), (32, 33)]
LEVELS = 3


@pytest.fixture(scope="module")
def lib():
    L = hb.load_library("dso_common", os.path.join(HERE, "host_logic", "dso_common_harness.cpp"))
    L.dso_make_levels.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.dso_interp33.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.dso_make_levels.restype = L.dso_interp33.restype = None
    return L


def _levels(lib, img, levels, pitch=0):
    H, W = img.shape
    rs = W + pitch
    src = np.full((H, rs), np.float32(np.nan))
    src[:, :W] = img
    out = np.zeros(sum((H >> l) * (W >> l) for l in range(levels)) * 4, np.float32)
    lib.dso_make_levels(hb.p(src), rs, W, H, levels, hb.p(out))
    lv, at = [], 0
    for l in range(levels):
        n = (H >> l) * (W >> l) * 4
        lv.append(out[at:at + n].reshape(H >> l, W >> l, 4))
        at += n
    return lv


@pytest.mark.parametrize("H,W", SHAPES)
def test_make_levels_is_the_coarse_oracles_pyramid(lib, H, W):
    """Level l depends only on the image's first (H >> l) << l rows and (W >> l) << l columns, so the oracle, which halves even sizes,
    restates it from that crop; a NaN and an infinite pixel exercise the non-finite-to-zero rule of the gradient."""
    rng = np.random.default_rng(100 * H + W)
    img = rng.uniform(0.0, 255.0, (H, W)).astype(np.float32)
    img[H // 2, W // 2], img[1, 2] = np.inf, np.nan
    for pitch in (0, 3):
        got = _levels(lib, img, LEVELS, pitch)
        for l in range(LEVELS):
            want = nco.make_images(img[:(H >> l) << l, :(W >> l) << l], l + 1)[l]
            assert want.shape == (H >> l, W >> l, 3) and nco.same_bits(got[l][:, :, :3], want), (l, pitch)
            assert not got[l][:, :, 3].any()
    assert np.isnan(got[0][:, :, 0]).sum() == 1 and np.isfinite(got[0][:, :, 1:3]).all() and got[0][:, :, 1:3].any()


@pytest.mark.parametrize("H,W", SHAPES)
def test_bilin_and_mix_are_the_window_oracles_interpolation(lib, H, W):
    """The window oracle interpolates inside linearize.  An identity precalc puts tap k of a point at (u + px_k, v + py_k); unit pattern
    weights, zero colours and affine terms, a Huber threshold and a gradient constant that never bind make resF, JIdx[0] and JIdx[1] of
    tap k exactly the interpolated colour, dx and dy.  Its window margin of 3 pixels leaves the pattern no room on 7 rows, so the test
    narrows the margin to the one pixel the interpolation itself needs; range checks are the callers' in the header as well."""
    rng = np.random.default_rng(7 * H + W)
    img = rng.uniform(0.0, 255.0, (H, W)).astype(np.float32)
    o = nwo.Oracle(H, W, (1.0, 1.0, 0.0, 0.0), prm=dict(outlier_th_sum_component=1e30, huber_th=3e38))
    o.wM3, o.hM3 = np.float32(W - 1), np.float32(H - 1)
    n = 40
    uv = np.stack([rng.uniform(3.2, W - 3.1, n), rng.uniform(3.2, H - 3.1, n)], axis=1).astype(np.float32)
    uv[0] = (np.float32(4.0), np.float32(3.5))                       # a whole-pixel column: dx = 0
    o.set_frames(0, img)
    o.set_points(np.zeros(n, np.int32), uv, np.zeros((n, 8), np.float32), np.ones((n, 8), np.float32), np.ones(n, np.float32))
    o.set_residuals(np.arange(n), np.zeros(n, np.int64))
    pc = np.zeros(27, np.float32)
    pc[[0, 4, 8]] = 1.0                                              # KRKi
    pc[[12, 16, 20]] = 1.0                                           # R0
    o.linearize(1, pc, np.array([np.float32(3e38)]))
    assert (o.r["new_state"] != nwo.OOB).all()
    xy = o.r["projected_to"].reshape(n * 8, 2).copy()
    want = np.stack([o.r["J"][:, nwo.J_RESF:nwo.J_RESF + 8], o.r["J"][:, nwo.J_JIDX:nwo.J_JIDX + 8], o.r["J"][:, nwo.J_JIDX + 8:nwo.J_JIDX + 16]],
                    axis=2).reshape(n * 8, 3)
    level0 = _levels(lib, img, 1)[0]
    got = np.zeros((n * 8, 3), np.float32)
    lib.dso_interp33(hb.p(level0), W, n * 8, hb.p(xy), hb.p(got))
    assert nco.same_bits(got, want) and np.isfinite(got).all() and got.any(axis=0).all()
    assert (xy != np.floor(xy)).any(axis=1).sum() > n                # fractions in both directions are in play


def test_dso_common_sources_are_build_inputs():
    """a header-only edit must rebuild the library (capi.build_inputs lists every .hip and .hpp of csrc); the shared level kernels are fp32 in the
    reference's order, so their translation unit is built without FMA contraction"""
    assert hc.is_build_input("eds_dso_image.hip") and hc.is_build_input("eds_dso_common.hpp")
    assert hc.contraction_off(hc.compile_line("eds_dso_image.o")) and hc.contraction_off(hc.resources_line("eds_dso_image.hip"))
    for f in ("eds_window.hpp", "eds_pixsel.hpp"):                   # the coarse tracker's header is no longer where pixels come from
        assert '#include "eds_coarse.hpp"' not in open(os.path.join(capi.CSRC, f)).read(), f


@pytest.mark.gpu
def test_device_helpers_against_serial_restatements(gpu, tmp_path):
    exe = str(tmp_path / "dso_common_check")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I" + capi.CSRC,
                           os.path.join(HERE, "cpp", "dso_common_check.hip"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "dso_common ok" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
