"""include/eds_hip_window.h, the companion header of the window optimiser's linearize: plain C like eds_hip.h, every function it
declares is exported by libeds_hip.so and listed in capi.WIN_EXPORTS, its defaults are the reference's settings table, its sources are
build inputs; and the stand-alone program of csrc/eds_window.hpp under g++ (tests/window_harness.py) over the cases and the hostile
inputs (no GPU needed: nothing here launches anything)."""
import ctypes as C
import importlib
import re

import window_cases as wc
import window_harness as wh
import header_checks as hc

capi = hc.capi
window = importlib.import_module("slam-eds_amd.window")

# reference src/utils/settings.cpp:91-127 and src/tracking/HessianBlocks.h:58-62
REFERENCE_SETTINGS = dict(outlier_th_sum_component=50.0 * 50.0, huber_th=9.0, affine_opt_mode_a=1e12, affine_opt_mode_b=1e8, scale_idepth=1.0,
                          scale_f=1.0, scale_c=1.0)


def test_window_c_program_links_every_declared_function(tmp_path):
    hc.link_and_run("eds_hip_window.h", hc.declared("eds_hip_window.h"), [
        "    eds_win_params p; eds_win_residual_out ro; eds_win_point_out po;",
        "    float x = 0; double d = 0; int32_t m[3] = {0, 0, 0};",
        "    if (eds_win_abi_version() != EDS_HIP_WINDOW_ABI_VERSION || EDS_HIP_WINDOW_ABI_VERSION != 1) return 3;",
        "    if (eds_abi_version() != 6) return 4;",
        "    eds_win_params_default(&p);",
        "    if (p.outlier_th_sum_component != 2500.0f || p.huber_th != 9.0f || p.affine_opt_mode_a != 1e12f || p.affine_opt_mode_b != 1e8f) return 5;",
        "    if (p.scale_idepth != 1.0f || p.scale_f != 1.0f || p.scale_c != 1.0f) return 5;",
        "    if (eds_win_set_params(0, &p) != EDS_ERR_INVALID || eds_win_get_params(0, &p) != EDS_ERR_INVALID) return 6;",
        "    if (eds_win_create(0, 48, 64, 8, 1, 1, 0) != EDS_ERR_INVALID) return 7;",
        "    if (eds_win_set_calib(0, 1, 1, 0, 0) != EDS_ERR_INVALID) return 8;",
        "    if (eds_win_set_frames(0, 0, 1, &x, 0, 0, 0) != EDS_ERR_INVALID || eds_win_get_frame(0, 0, &x) != EDS_ERR_INVALID) return 9;",
        "    if (eds_win_set_points(0, 0, 0, 0, 0, 0, 0, 0) != EDS_ERR_INVALID || eds_win_set_idepths(0, &x, &x) != EDS_ERR_INVALID) return 10;",
        "    if (eds_win_set_residuals(0, 0, 0, 0, 0, 0) != EDS_ERR_INVALID) return 11;",
        "    if (eds_win_linearize(0, 2, &x, &x, &d, m) != EDS_ERR_INVALID || eds_win_apply(0, 1) != EDS_ERR_INVALID) return 12;",
        "    if (eds_win_point_hessians(0, 0, 0, 0, 0, m) != EDS_ERR_INVALID) return 13;",
        "    if (eds_win_accumulate(0, 2, &d, &d, 0, 0, 0, 0, &d, &d, &d, &d, &d, m) != EDS_ERR_INVALID) return 13;",
        "    if (eds_win_acc_size(8) != 41888 || eds_win_acc_size(1) != 0 || eds_win_acc_size(9) != 0) return 13;",
        "    if (eds_win_get_residuals(0, &ro) != EDS_ERR_INVALID || eds_win_get_points(0, &po) != EDS_ERR_INVALID) return 14;",
        "    if (sizeof(eds_win_params) != 32 || EDS_WIN_MAX_FRAMES != 8 || EDS_WIN_PRECALC_FLOATS != 27 || EDS_WIN_J_WORDS != 74) return 15;",
        "    if (EDS_WIN_IN != 0 || EDS_WIN_OOB != 1 || EDS_WIN_OUTLIER != 2) return 16;",
        "    eds_win_destroy(0);"], tmp_path)


def test_defaults_equal_the_reference_settings():
    p = window.default_params()
    want = {k: C.c_float(v).value for k, v in REFERENCE_SETTINGS.items()}
    assert p.as_dict() == want == {k: C.c_float(v).value for k, v in wh.DEFAULTS.items()}
    assert [k for k, _ in window.Params._fields_][:-1] == list(REFERENCE_SETTINGS) == list(wh.PARAM_ORDER)
    assert window.RESIDUAL_FIELDS == wh.RESIDUAL_FIELDS and window.POINT_FIELDS == wh.POINT_FIELDS
    assert [k for k, _ in window.ResidualOut._fields_] == [k for k, _, _ in wh.RESIDUAL_FIELDS]
    assert (window.MAX_FRAMES, window.PRECALC_FLOATS, window.J_WORDS) == (8, 27, wh.J_WORDS)


def test_window_sources_are_build_inputs():
    for f in ("eds_window.hip", "eds_hip_window.h", "eds_window.hpp", "eds_device_owner.hpp", "eds_dso_common.hpp", "eds_dso_image.hip"):
        assert hc.is_build_input(f), f
    assert hc.contraction_off(hc.compile_line("eds_window.o")) and hc.contraction_off(hc.resources_line("eds_window.hip"))


def test_precalc_helper_forms_the_records_of_the_cases():
    """window.precalc is FrameFramePrecalc::set as tests/window_cases.py forms it, from the same poses"""
    import numpy as np
    c = wc.cases()["f3_5"]
    for h in range(c.F):
        for t in range(c.F):
            got = window.precalc(c.K, c.poses[h], c.poses[t], c.poses0[h], c.poses0[t], c.affs[h], c.affs[t], (c.exps[h], c.exps[t]))
            assert got.dtype == np.float32 and got.tobytes() == c.precalc[h * c.F + t].tobytes(), (h, t)
    adH, adT = window.adjoints(c.poses0, c.affs, c.exps)
    assert adH.shape == adT.shape == (c.F, c.F, 8, 8) and np.isfinite(adH).all()
    assert np.array_equal(adT[0, 1][:6, :6], np.eye(6)) and adT[0, 1][7, 7] == -1000.0 and np.allclose(adH[1, 1][:6, :6], -np.eye(6))


def test_standalone_program_builds_and_survives_the_hostile_inputs():
    """the program of the sanitizer run, built plainly: all cases twice (the second round after new idepths) plus NaN / inf /
    zero / huge precalc records and thresholds, idepths NaN / negative / 1e30, a point on every border pixel under the identity warp,
    thresholds 0 and NaN, a refused Huber threshold, the empty window; eds_win_accumulate's serial side in both rounds of every case
    and with NaN / inf (refused) and zero, -1, +-1e30, 1e-30, 1e300 adjoints, a point with two residuals towards one target (refused)"""
    out = wh.run_standalone(list(wc.cases().values()))
    m = re.search(r"window standalone: (\d+) cases; (\d+) residuals linearized, (\d+) IN, (\d+) OOB, (\d+) OUTLIER, (\d+) active added, (\d+) calls refused; (\d+) accumulates, (\d+) refused, (\d+) non-finite", out)
    assert m, out
    n_cases, res, n_in, n_oob, n_out, active, refused, accs, acc_refused, _ = (int(v) for v in m.groups())
    assert n_cases == len(wc.cases()) and res == n_in + n_oob + n_out and res > 10 ** 4 and n_in > 0 and n_oob > 0 and n_out > 0
    assert 0 < active and refused > 0 and accs > 2 * n_cases and acc_refused >= 2 * 2 * 4 + 2
