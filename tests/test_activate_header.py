"""include/eds_hip_activate.h, the companion header of the activation of immature points: plain C like eds_hip.h, every function it
declares is exported by libeds_hip.so and listed in capi.ACT_EXPORTS, every entry point answers a NULL handle with EDS_ERR_INVALID,
its struct is mirrored by activate.Params, and its sources are build inputs (no GPU needed: nothing here launches anything)."""
import ctypes as C
import importlib
import subprocess

import header_checks as hc

capi = hc.capi
activate = importlib.import_module("slam-eds_amd.activate")

DEFAULTS = dict(min_idepth_h_act=100.0, gn_its_on_point_activation=3, min_trace_quality=3.0, max_trace_pixel_interval=8.0, min_obs=1, scale_idepth=1.0)


def test_activate_header_is_c99_and_cxx11_clean(tmp_path):
    hc.compiles_clean("eds_hip_activate.h", "EDS_HIP_ACTIVATE_ABI_VERSION == 1 && EDS_HIP_IMMATURE_ABI_VERSION == 1 ? 0 : 1", tmp_path)


def test_activate_c_program_links_every_declared_function(tmp_path):
    hc.link_and_run("eds_hip_activate.h", hc.declared("eds_hip_activate.h"), [
        "    eds_act_params p;",
        "    float x = 0; int32_t t = 0; int m = 0;",
        "    if (eds_act_abi_version() != EDS_HIP_ACTIVATE_ABI_VERSION || EDS_HIP_ACTIVATE_ABI_VERSION != 1) return 3;",
        "    if (eds_abi_version() != 6 || eds_imm_abi_version() != 1) return 4;",
        "    eds_act_params_default(&p);",
        "    if (p.min_idepth_h_act != 100.0f || p.gn_its_on_point_activation != 3 || p.min_obs != 1 || p.scale_idepth != 1.0f) return 5;",
        "    if (eds_act_set_params(0, &p) != EDS_ERR_INVALID || eds_act_get_params(0, &p) != EDS_ERR_INVALID) return 6;",
        "    if (eds_act_set_calib(0, 1, 1, 0, 0) != EDS_ERR_INVALID) return 7;",
        "    if (eds_act_make_distance_map(0, 0, 1, &x, &x, 0, &t, &x, 0) != EDS_ERR_INVALID || eds_act_get_distance_map(0, &x) != EDS_ERR_INVALID) return 8;",
        "    if (eds_act_select(0, 0, 1, &x, &x, 0, 0.0f, &t) != EDS_ERR_INVALID || eds_act_optimize(0, 1, &x, &t) != EDS_ERR_INVALID) return 9;",
        "    if (eds_act_get(0, 0, &t, &x, &x, &x, &x, &t, &x) != EDS_ERR_INVALID) return 10;",
        "    if (eds_act_get_activated(0, 0, &m, 0, 0, 0, 0, 0, 0, 0, 0) != EDS_ERR_INVALID) return 11;",
        "    if (EDS_ACT_NONE != 0 || EDS_ACT_CHOSEN != 5 || EDS_ACT_ACTIVATED != 9 || EDS_ACT_NUM_FATES != 10 || EDS_ACT_MAX_FRAMES != 64) return 12;"], tmp_path)


def test_ctypes_struct_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "eds_hip_activate.h"\nint main(void) { printf("%d %d %d\\n", '
                   '(int)sizeof(eds_act_params), (int)offsetof(eds_act_params, min_obs), (int)offsetof(eds_act_params, scale_idepth)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", capi.INCLUDE, str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    P = activate.Params
    assert got == [C.sizeof(P), P.min_obs.offset, P.scale_idepth.offset]
    assert [k for k, _ in P._fields_] == list(DEFAULTS)
    assert (activate.NUM_FATES, activate.MAX_FRAMES, activate.PRECALC_FLOATS) == (10, 64, 14)


def test_activate_sources_are_build_inputs():
    """a header-only edit must rebuild the library (capi.build's staleness check); the fit is fp32 in the reference's order, so its
    translation unit is built without FMA contraction; the shared headers are prerequisites of every object"""
    for f in ("eds_activate.hip", "eds_hip_activate.h", "eds_activate.hpp", "eds_immature_internal.hpp", "eds_device_owner.hpp", "eds_dso_common.hpp"):
        assert hc.is_build_input(f), f
    assert hc.contraction_off(hc.compile_line("eds_activate.o")) and hc.resources_line("eds_activate.hip")


def test_the_controller_stays_within_its_range():
    assert activate.next_min_act_dist(100, 2000, 2.0) < 2.0 < activate.next_min_act_dist(4000, 2000, 2.0)
    assert activate.next_min_act_dist(0, 2000, 0.1) == 0.0 and activate.next_min_act_dist(10 ** 6, 2000, 3.9) == 4.0
