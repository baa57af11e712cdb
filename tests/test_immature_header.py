"""include/eds_hip_immature.h, the companion header of the immature-point trace: plain C like eds_hip.h, every function it declares is
exported by libeds_hip.so and listed in capi.IMM_EXPORTS, and its defaults are the reference's settings table (no GPU needed: nothing
here launches anything)."""
import ctypes as C
import importlib
import subprocess

import header_checks as hc

capi = hc.capi
immature = importlib.import_module("slam-eds_amd.immature")

# reference src/utils/settings.cpp:90-165
REFERENCE_SETTINGS = dict(max_pix_search=0.027, trace_stepsize=1.0, trace_gn_iterations=3, trace_gn_threshold=0.1, trace_extra_slack_on_th=1.2,
                          trace_slack_interval=1.5, trace_min_improvement_factor=2.0, min_trace_test_radius=2, huber_th=9.0,
                          outlier_th=12.0 * 12.0, outlier_th_sum_component=50.0 * 50.0, overall_energy_th_weight=1.0)


def test_immature_c_program_links_every_declared_function(tmp_path):
    hc.link_and_run("eds_hip_immature.h", hc.declared("eds_hip_immature.h"), [
        "    eds_imm_params p;", "    float x = 0; int32_t t = 0; int m = 0;",
        "    if (eds_imm_abi_version() != EDS_HIP_IMMATURE_ABI_VERSION || EDS_HIP_IMMATURE_ABI_VERSION != 1) return 3;",
        "    if (eds_abi_version() != 6) return 4;",
        "    eds_imm_params_default(&p);",
        "    if (p.trace_gn_iterations != 3 || p.min_trace_test_radius != 2 || p.outlier_th != 144.0f) return 5;",
        "    if (eds_imm_set_params(0, &p) != EDS_ERR_INVALID || eds_imm_get_params(0, &p) != EDS_ERR_INVALID) return 6;",
        "    if (eds_imm_create(0, 4, 4, 1, 1, 1, 0) != EDS_ERR_INVALID) return 7;",
        "    if (eds_imm_set_host_images(0, 0, 1, &x, 0, 0, 0) != EDS_ERR_INVALID) return 8;",
        "    if (eds_imm_trace(0, 0, 1, &t, &x, &x, &x, 0) != EDS_ERR_INVALID) return 9;",
        "    if (eds_imm_num_points(0, 0, &m) != EDS_ERR_INVALID || eds_imm_get_image(0, EDS_IMM_HOST_IMAGE, 0, &x) != EDS_ERR_INVALID) return 10;",
        "    if (EDS_IMM_GOOD != 0 || EDS_IMM_OOB != 1 || EDS_IMM_OUTLIER != 2 || EDS_IMM_SKIPPED != 3 || EDS_IMM_BADCONDITION != 4 ||",
        "        EDS_IMM_UNINITIALIZED != 5 || EDS_IMM_NUM_STATUS != 6) return 11;",
        "    eds_imm_destroy(0);"], tmp_path)


def test_defaults_equal_the_reference_settings():
    p = immature.default_params()
    want = {k: (v if isinstance(v, int) else C.c_float(v).value) for k, v in REFERENCE_SETTINGS.items()}
    assert p.as_dict() == want
    assert [k for k, _ in immature.Params._fields_] == list(REFERENCE_SETTINGS)


def test_ctypes_struct_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "eds_hip_immature.h"\nint main(void) { printf("%d %d %d\\n", '
                   '(int)sizeof(eds_imm_params), (int)offsetof(eds_imm_params, min_trace_test_radius), '
                   '(int)offsetof(eds_imm_params, overall_energy_th_weight)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", capi.INCLUDE, str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    P = immature.Params
    assert got == [C.sizeof(P), P.min_trace_test_radius.offset, P.overall_energy_th_weight.offset]


def test_immature_sources_are_build_inputs():
    """a header-only edit must rebuild the library (capi.build's staleness check); the trace is fp32 in the reference's order, so its
    translation unit is built without FMA contraction; the shared header is a prerequisite of every object"""
    for f in ("eds_immature.hip", "eds_hip_immature.h", "eds_immature.hpp", "eds_device_owner.hpp", "eds_dso_common.hpp"):
        assert hc.is_build_input(f), f
    assert hc.contraction_off(hc.compile_line("eds_immature.o"))
