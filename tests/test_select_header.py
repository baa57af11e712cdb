"""include/eds_hip_select.h, the header of the pixel selector: plain C like eds_hip.h, every function it declares is exported by
libeds_hip.so and listed in capi.SEL_EXPORTS, every entry point answers a NULL handle with EDS_ERR_INVALID, its structs are mirrored by
select.Params and select.Pass, its defaults are the reference's settings, and its sources are build inputs (no GPU needed: nothing here
launches anything)."""
import ctypes as C
import importlib
import subprocess

import numpy as np

import header_checks as hc

capi = hc.capi
select = importlib.import_module("slam-eds_amd.select")
immature = importlib.import_module("slam-eds_amd.immature")

# reference src/utils/settings.cpp:145-148
REFERENCE_SETTINGS = dict(min_grad_hist_cut=0.5, min_grad_hist_add=7.0, grad_downweight_per_level=0.75, select_direction_distribution=1)


def test_select_header_is_c99_and_cxx11_clean(tmp_path):
    hc.compiles_clean(("eds_hip_select.h", "eds_hip_immature.h"),
                      "EDS_HIP_SELECT_ABI_VERSION == 1 && EDS_HIP_IMMATURE_ABI_VERSION == 1 ? 0 : 1", tmp_path)


def test_select_declarations_equal_binding():
    assert "eds_imm_create_points_selected" in capi.IMM_EXPORTS


def test_select_c_program_links_every_declared_function(tmp_path):
    hc.link_and_run(("eds_hip_select.h", "eds_hip_immature.h"), hc.declared("eds_hip_select.h") + ["eds_imm_create_points_selected"], [
        "    eds_sel_params p;",
        "    eds_sel_pass ps;",
        "    float x = 0; int m = 0; uint8_t b = 0; int32_t t = 0;",
        "    if (eds_sel_abi_version() != EDS_HIP_SELECT_ABI_VERSION || EDS_HIP_SELECT_ABI_VERSION != 1) return 3;",
        "    if (eds_abi_version() != 6 || eds_imm_abi_version() != 1) return 4;",
        "    eds_sel_params_default(&p);",
        "    if (p.min_grad_hist_cut != 0.5f || p.min_grad_hist_add != 7.0f || p.grad_downweight_per_level != 0.75f || p.select_direction_distribution != 1) return 5;",
        "    if (eds_sel_set_params(0, &p) != EDS_ERR_INVALID || eds_sel_get_params(0, &p) != EDS_ERR_INVALID) return 6;",
        "    if (eds_sel_create(0, 16, 16, 0) != EDS_ERR_INVALID) return 7;",
        "    if (eds_sel_set_random_pattern(0, &b, 1) != EDS_ERR_INVALID || eds_sel_fill_reference_pattern(0, 1) != EDS_ERR_INVALID) return 8;",
        "    if (eds_sel_set_potential(0, 3) != EDS_ERR_INVALID || eds_sel_get_potential(0, &m) != EDS_ERR_INVALID) return 9;",
        "    if (eds_sel_set_image(0, &x, 0, 0, 0) != EDS_ERR_INVALID) return 10;",
        "    if (eds_sel_make_maps(0, 100.0f, 1, 1.0f, &m, &ps, 1, &m, 0) != EDS_ERR_INVALID) return 11;",
        "    if (eds_sel_get_map(0, &b) != EDS_ERR_INVALID || eds_sel_get_selection(0, &m, &t, &x) != EDS_ERR_INVALID) return 12;",
        "    if (eds_sel_get_level(0, 0, &x) != EDS_ERR_INVALID || eds_sel_get_thresholds(0, EDS_SEL_THS, &x) != EDS_ERR_INVALID) return 13;",
        "    if (eds_sel_get_scan_info(0, &m, &m) != EDS_ERR_INVALID) return 14;",
        "    if (eds_imm_create_points_selected(0, 0, 0, 0, 0, 1, 1, &b, &m) != EDS_ERR_INVALID) return 15;",
        "    if (EDS_SEL_THS != 0 || EDS_SEL_THS_SMOOTHED != 1 || EDS_SEL_MAX_POTENTIAL != 1073741824) return 16;",
        "    eds_sel_destroy(0);"], tmp_path)


def test_defaults_equal_the_reference_settings():
    p = select.default_params()
    want = {k: (v if isinstance(v, int) else C.c_float(v).value) for k, v in REFERENCE_SETTINGS.items()}
    assert p.as_dict() == want
    assert [k for k, _ in select.Params._fields_] == list(REFERENCE_SETTINGS)


def test_ctypes_structs_match_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "eds_hip_select.h"\nint main(void) { printf("%d %d %d %d\\n", '
                   '(int)sizeof(eds_sel_params), (int)offsetof(eds_sel_params, select_direction_distribution), (int)sizeof(eds_sel_pass), '
                   '(int)offsetof(eds_sel_pass, n4)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", capi.INCLUDE, str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    P, S = select.Params, select.Pass
    assert got == [C.sizeof(P), P.select_direction_distribution.offset, C.sizeof(S), S.n4.offset]
    assert (select.THS, select.THS_SMOOTHED, select.MAX_POTENTIAL) == (0, 1, 1 << 30)


def test_the_reference_pattern_is_the_constructors():
    """srand(3141592), then rand() & 0xFF: the library's table equals the C library's own draw, and two draws are equal"""
    import select_cases as sc
    a = select.reference_pattern(70 * 100)
    assert np.array_equal(a, sc.reference_table(70 * 100)) and np.array_equal(a, select.reference_pattern(70 * 100))
    assert np.array_equal(a[:32 * 32], select.reference_pattern(32 * 32))


def test_select_sources_are_build_inputs():
    """a header-only edit must rebuild the library (capi.build's staleness check); the selector is fp32 in the reference's order, so its
    translation unit is built without FMA contraction; the shared headers are prerequisites of every object"""
    for f in ("eds_pixsel.hip", "eds_hip_select.h", "eds_pixsel.hpp", "eds_pixsel_internal.hpp", "eds_device_owner.hpp", "eds_dso_common.hpp", "eds_dso_image.hip"):
        assert hc.is_build_input(f), f
    assert hc.contraction_off(hc.compile_line("eds_pixsel.o")) and hc.resources_line("eds_pixsel.hip")
