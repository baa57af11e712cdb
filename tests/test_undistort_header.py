"""include/eds_hip_undistort.h, the header of the undistorter: plain C like eds_hip.h, every function it declares is exported by
libeds_hip.so and listed in capi.UND_EXPORTS, every entry point answers a NULL handle with EDS_ERR_INVALID, its structs are mirrored by
undistort.Geometry and undistort.Settings, its defaults are the reference's settings, and its sources are build inputs (no GPU needed:
nothing here launches anything)."""
import ctypes as C
import importlib
import os
import re
import subprocess

import header_checks as hc

REFERENCE_SETTINGS_CPP = "/root/reference/src/utils/settings.cpp"
capi = hc.capi
und = importlib.import_module("slam-eds_amd.undistort")

# reference src/utils/settings.cpp:117-118
REFERENCE_SETTINGS = dict(photometric_calibration=2, use_exposure=1)


def test_undistort_header_is_c99_and_cxx11_clean(tmp_path):
    hc.compiles_clean(("eds_hip_undistort.h", "eds_hip_select.h"),
                      "EDS_HIP_UNDISTORT_ABI_VERSION == 1 && EDS_HIP_SELECT_ABI_VERSION == 1 ? 0 : 1", tmp_path)


def test_undistort_c_program_links_every_declared_function(tmp_path):
    hc.link_and_run("eds_hip_undistort.h", hc.declared("eds_hip_undistort.h"), [
        "    eds_und_settings s;",
        "    eds_und_geometry g;",
        "    eds_und* u = (eds_und*)&g;",
        "    double K[9]; float x = 0; int m = 0; uint8_t b = 0; const float* d = 0; int64_t rs = 0;",
        "    if (eds_und_abi_version() != EDS_HIP_UNDISTORT_ABI_VERSION || EDS_HIP_UNDISTORT_ABI_VERSION != 1) return 3;",
        "    if (eds_abi_version() != 6) return 4;",
        "    eds_und_settings_default(&s);",
        "    if (s.photometric_calibration != 2 || s.use_exposure != 1) return 5;",
        "    if (eds_und_create(0, 0, 1, &u) != EDS_ERR_INVALID || u != 0 || eds_und_create(0, &g, 1, 0) != EDS_ERR_INVALID) return 6;",
        "    if (eds_und_get_K(0, K) != EDS_ERR_INVALID || eds_und_get_map(0, &x, &x) != EDS_ERR_INVALID) return 7;",
        "    if (eds_und_is_passthrough(0, &m) != EDS_ERR_INVALID || eds_und_set_map(0, &x, &x) != EDS_ERR_INVALID) return 8;",
        "    if (eds_und_set_photometric(0, &x, 256, &b, EDS_UND_U8) != EDS_ERR_INVALID) return 9;",
        "    if (eds_und_set_settings(0, &s) != EDS_ERR_INVALID || eds_und_get_settings(0, &s) != EDS_ERR_INVALID) return 10;",
        "    if (eds_und_set_form(0, EDS_UND_FORM_FUSED) != EDS_ERR_INVALID || eds_und_get_form(0, &m) != EDS_ERR_INVALID) return 11;",
        "    if (eds_und_process(0, 0, 1, &b, EDS_UND_U8, 0, 0, 0, &x, 1.0f, &x) != EDS_ERR_INVALID) return 12;",
        "    if (eds_und_image(0, 0, &d, &rs) != EDS_ERR_INVALID || eds_und_get_image(0, 0, &x) != EDS_ERR_INVALID) return 13;",
        "    if (EDS_UND_MODEL_FOV != 0 || EDS_UND_MODEL_RADTAN != 1 || EDS_UND_MODEL_EQUIDISTANT != 2 || EDS_UND_MODEL_KB != 3 || EDS_UND_MODEL_PINHOLE != 4) return 14;",
        "    if (EDS_UND_OUT_CROP != 0 || EDS_UND_OUT_NONE != 1 || EDS_UND_OUT_GIVEN != 2 || EDS_UND_OUT_FULL != 3) return 15;",
        "    if (EDS_UND_U8 != 0 || EDS_UND_U16 != 1 || EDS_UND_FORM_FUSED != 0 || EDS_UND_FORM_TWO_PASS != 1 || EDS_UND_FORM_AUTO != 2 || EDS_UND_MAX_SLOTS != 16) return 16;",
        "    eds_und_destroy(0);"], tmp_path)


def test_invalid_geometries_are_refused_before_any_device_is_touched():
    """what eds_und_create refuses it refuses on the host: these answers need no GPU"""
    L = und._lib()
    good = dict(model=und.MODEL_PINHOLE, pars=[30.0, 30.0, 19.5, 15.5, 0.0], w_org=40, h_org=32, out_mode=und.OUT_CROP, w=36, h=28)
    for change, code in ((dict(out_mode=und.OUT_FULL), capi.ERR_INVALID), (dict(w=7), capi.ERR_INVALID), (dict(h_org=8193), capi.ERR_INVALID),
                         (dict(model=5), capi.ERR_INVALID), (dict(out_mode=und.OUT_NONE), capi.ERR_INVALID),
                         (dict(pars=[30.0, float("nan"), 19.5, 15.5, 0.0]), capi.ERR_INVALID),
                         (dict(pars=[30.0, 30.0, 5000.0, 15.5, 0.0]), capi.ERR_NOT_USABLE)):
        h = C.c_void_p(1)
        g = und.geometry(**dict(good, **change))
        assert L.eds_und_create(0, C.byref(g), 1, C.byref(h)) == code and not h.value, change
        assert capi.last_error()
    for slots in (0, 17):
        h = C.c_void_p(1)
        assert L.eds_und_create(0, C.byref(und.geometry(**good)), slots, C.byref(h)) == capi.ERR_INVALID and not h.value


def test_defaults_equal_the_reference_settings():
    s = und.default_settings()
    assert s.as_dict() == REFERENCE_SETTINGS
    assert [k for k, _ in und.Settings._fields_] == list(REFERENCE_SETTINGS)
    import np_undistort_oracle as uo
    assert uo.SETTINGS == REFERENCE_SETTINGS


def test_defaults_are_those_of_the_reference_tree():
    """where the reference tree is present the two settings are read from its settings.cpp; elsewhere the literals above stand"""
    if not os.path.exists(REFERENCE_SETTINGS_CPP):
        return
    text = open(REFERENCE_SETTINGS_CPP).read()
    mode = re.search(r"int\s+setting_photometricCalibration\s*=\s*(\d+)\s*;", text)
    use = re.search(r"bool\s+setting_useExposure\s*=\s*(true|false)\s*;", text)
    assert int(mode.group(1)) == REFERENCE_SETTINGS["photometric_calibration"]
    assert (use.group(1) == "true") == bool(REFERENCE_SETTINGS["use_exposure"])


def test_ctypes_structs_match_the_header(tmp_path):
    src = tmp_path / "sz.c"
    fields = ["model", "pars", "w_org", "h_org", "out_mode", "out_pars", "w", "h"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "eds_hip_undistort.h"\nint main(void) { printf("%d %d %d %d' + " %d" * len(fields) +
                   '\\n", (int)sizeof(eds_und_geometry), (int)sizeof(eds_und_settings), (int)offsetof(eds_und_settings, photometric_calibration), '
                   "(int)offsetof(eds_und_settings, use_exposure), " + ", ".join(f"(int)offsetof(eds_und_geometry, {f})" for f in fields) + "); return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", capi.INCLUDE, str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    G, S = und.Geometry, und.Settings
    assert [k for k, _ in G._fields_] == fields
    assert got == [C.sizeof(G), C.sizeof(S), S.photometric_calibration.offset, S.use_exposure.offset] + [getattr(G, f).offset for f in fields]
    assert (und.MODEL_FOV, und.MODEL_RADTAN, und.MODEL_EQUIDISTANT, und.MODEL_KB, und.MODEL_PINHOLE) == (0, 1, 2, 3, 4)
    assert (und.OUT_CROP, und.OUT_NONE, und.OUT_GIVEN, und.OUT_FULL, und.U8, und.U16, und.FORM_FUSED, und.FORM_TWO_PASS, und.FORM_AUTO, und.MAX_SLOTS) == (0, 1, 2, 3, 0, 1, 0, 1, 2, 16)


def test_undistort_sources_are_build_inputs():
    """a header-only edit must rebuild the library (capi.build's staleness check); the per-frame path is fp32 in the reference's order, so
    its translation unit is built without FMA contraction; the shared headers are prerequisites of every object"""
    for f in ("eds_undistort.hip", "eds_hip_undistort.h", "eds_undistort.hpp", "eds_device_owner.hpp", "eds_dso_common.hpp"):
        assert hc.is_build_input(f), f
    assert hc.contraction_off(hc.compile_line("eds_undistort.o")) and hc.resources_line("eds_undistort.hip")
