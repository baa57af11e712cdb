"""include/eds_hip_activate.h, the companion header of the activation of immature points: plain C like eds_hip.h, every function it
declares is exported by libeds_hip.so and listed in capi.ACT_EXPORTS, every entry point answers a NULL handle with EDS_ERR_INVALID,
its struct is mirrored by activate.Params, and its sources are build inputs (no GPU needed: nothing here launches anything)."""
import ctypes as C
import importlib
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "eds_hip_activate.h")
capi = importlib.import_module("slam-eds_amd.capi")
activate = importlib.import_module("slam-eds_amd.activate")

DEFAULTS = dict(min_idepth_h_act=100.0, gn_its_on_point_activation=3, min_trace_quality=3.0, max_trace_pixel_interval=8.0, min_obs=1, scale_idepth=1.0)


def _declared_functions():
    text = re.sub(r"/\*.*?\*/", " ", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(eds_act_[a-z0-9_]+)\s*\(", text)))


def test_activate_header_is_c99_and_cxx11_clean(tmp_path):
    for std, cc, ext in (("-std=c99", "gcc", "c"), ("-std=c++11", "g++", "cpp")):
        src = tmp_path / ("inc." + ext)
        src.write_text('#include "eds_hip_activate.h"\nint main(void) { return EDS_HIP_ACTIVATE_ABI_VERSION == 1 && EDS_HIP_IMMATURE_ABI_VERSION == 1 ? 0 : 1; }\n')
        subprocess.check_call([cc, std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                               "-o", str(tmp_path / "inc.o")])


def test_activate_declarations_equal_binding():
    assert _declared_functions() == sorted(capi.ACT_EXPORTS)
    others = (set(capi.EXPORTS) | set(capi.DEPTH_EXPORTS) | set(capi.KLT_EXPORTS) | set(capi.EPI_EXPORTS) | set(capi.DEV_EXPORTS) |
              set(capi.KFP_EXPORTS) | set(capi.KFS_EXPORTS) | set(capi.IMM_EXPORTS) | set(capi.CT_EXPORTS) | set(capi.WIN_EXPORTS) | set(capi.WSV_EXPORTS))
    assert not set(capi.ACT_EXPORTS) & others
    assert len(set(capi.ACT_EXPORTS)) == len(capi.ACT_EXPORTS)


def test_activate_c_program_links_every_declared_function(tmp_path):
    capi.build()
    names = _declared_functions()
    lines = ['#include <stdio.h>', '#include "eds_hip_activate.h"', "int main(void) {", "    const void* f[] = {"]
    lines += [f"        (const void*)(size_t)&{n}," for n in names]
    lines += ["    };", "    size_t i, n = sizeof(f) / sizeof(f[0]);", "    eds_act_params p;", "    float x = 0; int32_t t = 0; int m = 0;",
              "    for (i = 0; i < n; ++i) if (!f[i]) return 2;",
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
              "    if (EDS_ACT_NONE != 0 || EDS_ACT_CHOSEN != 5 || EDS_ACT_ACTIVATED != 9 || EDS_ACT_NUM_FATES != 10 || EDS_ACT_MAX_FRAMES != 64) return 12;",
              '    printf("%d functions\\n", (int)n);', "    return 0;", "}"]
    src = tmp_path / "link.c"
    src.write_text("\n".join(lines) + "\n")
    libdir = os.path.dirname(capi.LIB_PATH)
    exe = tmp_path / "link"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-leds_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    assert f"{len(names)} functions" in subprocess.check_output([str(exe)], text=True)
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = set(re.findall(r"\s[TW]\s+(\S+)", out))
    assert set(names) <= exported


def test_ctypes_struct_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "eds_hip_activate.h"\nint main(void) { printf("%d %d %d\\n", '
                   '(int)sizeof(eds_act_params), (int)offsetof(eds_act_params, min_obs), (int)offsetof(eds_act_params, scale_idepth)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    P = activate.Params
    assert got == [C.sizeof(P), P.min_obs.offset, P.scale_idepth.offset]
    assert [k for k, _ in P._fields_] == list(DEFAULTS)
    assert (activate.NUM_FATES, activate.MAX_FRAMES, activate.PRECALC_FLOATS) == (10, 64, 14)


def test_activate_sources_are_build_inputs():
    """a header-only edit must rebuild the library (capi.build's staleness check); the fit is fp32 in the reference's order, so its
    translation unit is built without FMA contraction; the shared headers are prerequisites of every object"""
    import inspect
    assert "eds_hip_activate.h" in inspect.getsource(capi.build)
    mk = open(os.path.join(capi.CSRC, "Makefile")).read()
    for f in ("eds_activate.hip", "eds_hip_activate.h", "eds_activate.hpp", "eds_immature_internal.hpp", "eds_device_owner.hpp", "eds_dso_common.hpp"):
        assert f in mk, f
    assert "eds_activate.o: HIPFLAGS += -ffp-contract=off" in mk
    assert "-c eds_activate.hip -o /dev/null" in mk


def test_the_controller_stays_within_its_range():
    assert activate.next_min_act_dist(100, 2000, 2.0) < 2.0 < activate.next_min_act_dist(4000, 2000, 2.0)
    assert activate.next_min_act_dist(0, 2000, 0.1) == 0.0 and activate.next_min_act_dist(10 ** 6, 2000, 3.9) == 4.0
