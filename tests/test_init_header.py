"""include/eds_hip_init.h, the companion header of DSO's initialiser: plain C like eds_hip.h, every function it declares is exported by
libeds_hip.so, listed in capi.INI_EXPORTS and bound in slam-eds_amd/init.py, its defaults are the reference's, every creator and setter
refuses its arguments before it touches the device, and csrc/eds_init.hpp's own atan is within the ulps it states of libm (no GPU
needed: nothing here launches anything)."""
import ctypes as C
import importlib
import math
import os
import re

import numpy as np

import init_harness as ih
import header_checks as hc

capi = hc.capi
init = importlib.import_module("slam-eds_amd.init")

# reference src/init/CoarseInitializer.cpp:58-61, :79-86; src/utils/settings.cpp:90, :127; src/tracking/HessianBlocks.h:59-65
REFERENCE = dict(huber_th=9.0, outlier_th=144.0, alpha_k=6.25, alpha_w=22500.0, reg_weight=0.8, coupling_weight=1.0, fix_affine=1,
                 max_iterations=[5, 5, 10, 30, 50], scale_xi_rot=1.0, scale_xi_trans=1.0, scale_a=10.0, scale_b=1000.0)


def test_init_declarations_equal_binding():
    capi.build()
    L = init._lib()
    for name in capi.INI_EXPORTS:
        assert getattr(L, name).argtypes is not None or name == "eds_ini_abi_version", name


def test_init_c_program_links_every_function_and_arguments_are_refused_before_the_device(tmp_path):
    """a C program calls every setter and creator with arguments that must be refused: no device is needed to be told so"""
    hc.link_and_run("eds_hip_init.h", hc.declared("eds_hip_init.h"), [
        "    eds_ini_params p; eds_ini_result r; eds_ini_point pt; eds_ini* h = 0;",
        "    float x = 0, uv[4] = {3.1f, 3.1f, 4.1f, 3.1f}; double d[12] = {0}; int32_t m = 0, nb[20], par[2];",
        "    if (eds_ini_abi_version() != EDS_HIP_INIT_ABI_VERSION || EDS_HIP_INIT_ABI_VERSION != 1) return 3;",
        "    eds_ini_params_default(&p);",
        "    if (p.huber_th != 9.0f || p.outlier_th != 144.0f || p.alpha_k != 6.25f || p.alpha_w != 22500.0f || p.reg_weight != 0.8f) return 4;",
        "    if (p.coupling_weight != 1.0f || p.fix_affine != 1 || p.max_iterations[4] != 50 || p.scale_a != 10.0f || p.scale_b != 1000.0f) return 5;",
        "    if (eds_ini_create(0, 64, 64, 5, 100, 0) != EDS_ERR_INVALID || eds_ini_create(0, 64, 64, 6, 100, &h) != EDS_ERR_INVALID) return 6;",
        "    if (eds_ini_create(0, 50, 64, 3, 100, &h) != EDS_ERR_INVALID || eds_ini_create(0, 48, 64, 3, 0, &h) != EDS_ERR_INVALID) return 7;",
        "    if (eds_ini_create(0, 48, 64, 3, EDS_INI_MAX_POINTS + 1, &h) != EDS_ERR_INVALID || h) return 8;",
        "    if (eds_ini_set_params(0, &p) != EDS_ERR_INVALID || eds_ini_get_params(0, &p) != EDS_ERR_INVALID) return 9;",
        "    if (eds_ini_set_calib(0, 1, 1, 0, 0) != EDS_ERR_INVALID || eds_ini_set_first(0, &x, 0, 0, 1) != EDS_ERR_INVALID) return 10;",
        "    if (eds_ini_set_pose(0, d, d) != EDS_ERR_INVALID || eds_ini_set_points(0, 0, &x, 0, 0, &m) != EDS_ERR_INVALID) return 11;",
        "    if (eds_ini_set_points_selected(0, 0, &m) != EDS_ERR_INVALID || eds_ini_set_neighbours(0, 0, nb, par) != EDS_ERR_INVALID) return 12;",
        "    if (eds_ini_track_frame(0, &x, 0, 0, 1, 5, &r) != EDS_ERR_INVALID || eds_ini_get_schedule_depth(0, 0, &m) != EDS_ERR_INVALID) return 13;",
        "    if (eds_ini_get_points(0, 0, &pt, &m) != EDS_ERR_INVALID || eds_ini_get_jb(0, 0, 0, &x) != EDS_ERR_INVALID) return 14;",
        "    if (eds_ini_get_level(0, 0, 0, &x) != EDS_ERR_INVALID || eds_ini_get_kernel_ms(0, &x) != EDS_ERR_INVALID) return 15;",
        "    if (eds_ini_make_nn(2, 0, 0, 0, nb, 0) != EDS_ERR_INVALID || eds_ini_make_nn(2, uv, 0, 0, nb, par) != EDS_ERR_INVALID) return 16;",
        "    if (eds_ini_make_nn(2, uv, 0, 0, nb, 0) != EDS_OK || nb[0] != 0 || nb[1] != 1 || nb[2] != -1 || nb[10] != 1 || nb[11] != 0) return 17;",
        "    if (sizeof(eds_ini_point) != 64 || sizeof(eds_ini_result) != 712 || sizeof(eds_ini_params) != 64 || EDS_INI_MAX_LEVELS != 5) return 18;",
        "    eds_ini_destroy(0);"], tmp_path)


def test_defaults_equal_the_reference_and_the_records_agree():
    p = init.default_params()
    want = {k: (C.c_float(v).value if isinstance(v, float) else v) for k, v in REFERENCE.items()}
    assert p.as_dict() == want
    assert [k for k, _ in init.Params._fields_] == list(REFERENCE) == list(ih.PARAMS.names)
    assert C.sizeof(init.Params) == ih.PARAMS.itemsize == 64
    assert init.POINT == ih.POINT and init.RESULT == ih.RESULT
    h = ih.default_params()[0]
    assert {k: (h[k].tolist()) for k in ih.PARAMS.names} == want
    assert (init.MAX_LEVELS, init.MAX_DECISIONS, init.MAX_ITERATIONS, init.MAX_POINTS, init.NEIGHBOURS) == (5, 512, 100, 65536, 10)


def test_init_sources_are_build_inputs():
    for f in ("eds_init.hip", "eds_hip_init.h", "eds_init.hpp", "eds_dso_common.hpp"):
        assert hc.is_build_input(f), f
    assert hc.contraction_off(hc.compile_line("eds_init.o")) and hc.contraction_off(hc.resources_line("eds_init.hip"))
    hip = open(os.path.join(capi.CSRC, "eds_init.hip")).read()
    assert "eds_device_owner.hpp" in open(os.path.join(capi.CSRC, "eds_capi_internal.hpp")).read() or "eds_device_owner.hpp" in hip
    assert "edscapi::DeviceOwner own;" in hip and "hipMalloc" not in hip and "hipFree" not in hip


def test_every_launch_and_wait_of_the_initialiser_is_counted():
    """eds_ini_result.launches / .waits are differences of the handle's counters, which INI_LAUNCH, ini_wait and ini_read_back advance:
    the file must not launch, wait or copy synchronously anywhere else"""
    hip = open(os.path.join(capi.CSRC, "eds_init.hip")).read()
    assert hip.count("hipLaunchKernelGGL(") == 1 and "++(h)->n_launches;" in hip
    assert hip.count("hipStreamSynchronize(") == 1 and hip.count("edscapi::read_back(") == 1 and hip.count("++h->n_waits;") == 2
    for other in ("hipDeviceSynchronize", "hipEventSynchronize", "hipStreamWaitEvent", "hipMemcpy(", "hipMemcpy2D(", "hipMemset(", "<<<"):
        assert other not in hip, other
    assert "h->n_launches - launches0" in hip and "h->n_waits - waits0" in hip


def _ulps(got, want):
    want = np.asarray(want, dtype=np.float64)
    return np.abs(got - want) / np.spacing(np.abs(want))


def test_own_atan_is_within_the_stated_ulps_of_libm():
    """logAndTheta's argument is n / w of a unit quaternion: any real number.  The samples cover the small angles of a tracked motion
    densely, every reduction interval and its boundaries, the switch at |x| = 1, and the huge and tiny ends (measured: 2 ulps)"""
    rng = np.random.default_rng(0)
    bound = ih.load_harness().ini_atan_max_ulp()
    hdr = open(os.path.join(capi.CSRC, "eds_coarse.hpp")).read()     # beside SINCOS_MAX_ULP / EXP_MAX_ULP
    assert f"ATAN_MAX_ULP = {bound};" in hdr and bound == 2
    edges = np.concatenate([(np.arange(0, 17) + 0.5) / 8.0, np.arange(0, 9) / 8.0, 8.0 / (np.arange(1, 17) + 0.5)])
    x = np.concatenate([rng.uniform(-0.2, 0.2, 100000), rng.uniform(-1, 1, 100000), rng.uniform(-16, 16, 100000), 10.0 ** rng.uniform(-300, 300, 50000),
                        -(10.0 ** rng.uniform(-20, 20, 50000)), edges, -edges, np.nextafter(edges, 0), np.nextafter(edges, 10), [0.0, 1.0, -1.0, 1e-320]])
    got = ih.atan(x)
    want = np.array([math.atan(v) for v in x])
    nz = want != 0
    worst = _ulps(got[nz], want[nz]).max()
    print(f"max ulps: atan {worst:.2f}")
    assert worst <= bound and (got[~nz] == 0).all()
    a = ih.atan(np.array([np.nan, np.inf, -np.inf]))
    assert np.isnan(a[0]) and a[1] == math.pi / 2 and a[2] == -math.pi / 2


def test_log_upsilon_agrees_with_a_closed_form_over_libm():
    import coarse_cases as cc
    import np_init_oracle as no
    rng = np.random.default_rng(1)
    for _ in range(200):
        T = cc.se3(rng.normal(0, 1, 3) * 10.0 ** rng.uniform(-6, 0.3), rng.normal(0, 1, 3))
        got, want = ih.log_upsilon(T), no.se3_log_upsilon(T[:, :3], T[:, 3])
        assert np.abs(got - want).max() <= 1e-9 * max(1.0, np.abs(want).max()), (T, got, want)
    assert np.array_equal(ih.log_upsilon(cc.se3((0, 0, 0), (1, 2, 3))), [1.0, 2.0, 3.0])


def test_standalone_program_builds_and_survives_the_hostile_inputs():
    """the program of the sanitizer run, built plainly: NaN / inf pixels and exposures, tables thinned to -1"""
    out = ih.run_standalone()
    m = re.search(r"init standalone: (\d+) tracks, (\d+) iterations, (\d+) points", out)
    assert m and int(m.group(1)) >= 18 and int(m.group(2)) > 100, out
