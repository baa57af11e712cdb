"""include/eds_hip_winsolve.h, the companion header of the window's solve: plain C like eds_hip.h, every function it declares is
exported by libeds_hip.so and listed in capi.WSV_EXPORTS, every entry point answers a NULL handle with EDS_ERR_INVALID, its sources are
build inputs, eds_hip_window.h declares what it declared before; and the stand-alone program of csrc/eds_winsolve.hpp under g++
(tests/winsolve_harness.py) over the cases and the hostile inputs (no GPU needed: nothing here launches anything)."""
import importlib
import os
import re
import subprocess

import winsolve_cases as wsc
import winsolve_harness as wsh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "eds_hip_winsolve.h")
capi = importlib.import_module("slam-eds_amd.capi")
winsolve = importlib.import_module("slam-eds_amd.winsolve")


def _declared(path, prefix):
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(" + prefix + r"[a-z0-9_]+)\s*\(", text)))


def test_winsolve_header_is_c99_and_cxx11_clean(tmp_path):
    for std, cc_, ext in (("-std=c99", "gcc", "c"), ("-std=c++11", "g++", "cpp")):
        src = tmp_path / ("inc." + ext)
        src.write_text('#include "eds_hip_winsolve.h"\nint main(void) { return EDS_HIP_WINSOLVE_ABI_VERSION == 1 && EDS_HIP_WINDOW_ABI_VERSION == 1 ? 0 : 1; }\n')
        subprocess.check_call([cc_, std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                               "-o", str(tmp_path / "inc.o")])


def test_winsolve_declarations_equal_binding():
    assert _declared(HDR, "eds_wsv_") == sorted(capi.WSV_EXPORTS)
    others = (set(capi.EXPORTS) | set(capi.DEPTH_EXPORTS) | set(capi.KLT_EXPORTS) | set(capi.EPI_EXPORTS) | set(capi.DEV_EXPORTS) |
              set(capi.KFP_EXPORTS) | set(capi.KFS_EXPORTS) | set(capi.IMM_EXPORTS) | set(capi.CT_EXPORTS) | set(capi.WIN_EXPORTS))
    assert not set(capi.WSV_EXPORTS) & others
    assert len(set(capi.WSV_EXPORTS)) == len(capi.WSV_EXPORTS)
    # the window header declares exactly what it declared: nothing of this header leaked into it
    assert _declared(os.path.join(ROOT, "include", "eds_hip_window.h"), "eds_win_") == sorted(capi.WIN_EXPORTS)
    assert not _declared(os.path.join(ROOT, "include", "eds_hip_window.h"), "eds_wsv_")
    # the mode bits are the reference's (src/utils/settings.h:35-46)
    text = open(HDR).read()
    for name, bit in (("SVD", 1), ("ORTHOGONALIZE_SYSTEM", 2), ("ORTHOGONALIZE_POINTMARG", 4), ("ORTHOGONALIZE_FULL", 8), ("SVD_CUT7", 16),
                      ("REMOVE_POSEPRIOR", 32), ("USE_GN", 64), ("FIX_LAMBDA", 128), ("ORTHOGONALIZE_X", 256), ("MOMENTUM", 512),
                      ("STEPMOMENTUM", 1024), ("ORTHOGONALIZE_X_LATER", 2048)):
        assert re.search(rf"#define EDS_WSV_SOLVER_{name} {bit}\b", text), name
        assert getattr(winsolve, "SOLVER_" + name) == bit
    assert winsolve.SOLVER_DEFAULT == 128 | 2048 == wsc.DEFAULT


def test_winsolve_c_program_links_every_declared_function(tmp_path):
    capi.build()
    names = _declared(HDR, "eds_wsv_")
    lines = ['#include <stdio.h>', '#include "eds_hip_winsolve.h"', "int main(void) {", "    const void* f[] = {"]
    lines += [f"        (const void*)(size_t)&{n}," for n in names]
    lines += ["    };", "    size_t i, n = sizeof(f) / sizeof(f[0]);", "    eds_wsv_stats st; eds_wsv_out out;",
              "    float x = 0; double d[4] = {0, 0, 0, 0}; int32_t m[3] = {0, 0, 0};",
              "    for (i = 0; i < n; ++i) if (!f[i]) return 2;",
              "    if (eds_wsv_abi_version() != EDS_HIP_WINSOLVE_ABI_VERSION || EDS_HIP_WINSOLVE_ABI_VERSION != 1) return 3;",
              "    if (eds_abi_version() != 6 || eds_win_abi_version() != 1) return 4;",
              "    if (eds_wsv_set_state(0, 2, d, d, d, d, d, d, d, &x, &x) != EDS_ERR_INVALID) return 5;",
              "    if (eds_wsv_fix_linearization(0, m) != EDS_ERR_INVALID) return 6;",
              "    if (eds_wsv_solve(0, 0, 0.0, 0, 1, d, d, d, d, d, d, &st) != EDS_ERR_INVALID) return 7;",
              "    if (eds_wsv_backup_idepths(0) != EDS_ERR_INVALID || eds_wsv_step_idepths(0, 1.0f) != EDS_ERR_INVALID) return 8;",
              "    if (eds_wsv_get_steps(0, &x) != EDS_ERR_INVALID) return 9;",
              "    if (eds_wsv_l_energy(0, d) != EDS_ERR_INVALID || eds_wsv_m_energy(0, d, d, d) != EDS_ERR_INVALID) return 10;",
              "    if (eds_wsv_marginalize_points(0, m, 1.0f, 1.0, d, d, m) != EDS_ERR_INVALID) return 11;",
              "    if (eds_wsv_get(0, &out) != EDS_ERR_INVALID) return 12;",
              "    if (sizeof(eds_wsv_stats) != 24 || sizeof(eds_wsv_out) != 12 * sizeof(void*)) return 13;",
              "    if (EDS_WSV_SOLVER_FIX_LAMBDA != 128 || EDS_WSV_SOLVER_ORTHOGONALIZE_X_LATER != 2048) return 14;",
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


def test_winsolve_binding_matches_the_harness():
    assert [k for k, _, _ in winsolve.OUT_FIELDS] == [k for k, _, _ in wsh.OUT_FIELDS] == [k for k, _ in winsolve.Out._fields_]
    assert winsolve.SYSTEM_FIELDS == wsh.SYSTEM_FIELDS
    assert [k for k, _ in winsolve.Stats._fields_] == [k for k, _ in wsh.Stats._fields_]
    assert (capi.ERR_INVALID, capi.ERR_NOT_USABLE, capi.ERR_STATE) == (wsh.INVALID, wsh.NOT_USABLE, wsh.STATE)
    assert (wsh.PRIOR_FAC, wsh.WEIGHT_FAC, wsh.DEFAULT_MODE) == (wsc.PRIOR_FAC, wsc.WEIGHT_FAC, wsc.DEFAULT)


def test_winsolve_sources_are_build_inputs():
    import inspect
    assert "eds_hip_winsolve.h" in inspect.getsource(capi.build)
    mk = open(os.path.join(capi.CSRC, "Makefile")).read()
    for f in ("eds_winsolve.hip", "eds_hip_winsolve.h", "eds_winsolve.hpp", "eds_window_internal.hpp", "eds_device_owner.hpp", "eds_dso_common.hpp"):
        assert f in mk, f
    assert "eds_winsolve.o: HIPFLAGS += -ffp-contract=off" in mk
    assert "-ffp-contract=off -Rpass-analysis=kernel-resource-usage -c eds_winsolve.hip" in mk
    # the definition of eds_win lives in the internal header both translation units include
    assert "struct eds_win {" in open(os.path.join(capi.CSRC, "eds_window_internal.hpp")).read()
    for f in ("eds_window.hip", "eds_winsolve.hip"):
        text = open(os.path.join(capi.CSRC, f)).read()
        assert '#include "eds_window_internal.hpp"' in text and "struct eds_win {" not in text, f


def test_standalone_program_builds_and_survives_the_hostile_inputs():
    """the program of the sanitizer run, built plainly: every case through four rounds of solves in both assembly branches
    with both energies and the step, a refused marginalisation, every residual linearized, a marginalisation and a solve after it; then
    every refused mode bit; NaN / +-inf / 0 / +-1e30 / 1e300 in HM, bM, the projector, the adjoints, the deltas and the priors (refused, or
    run to the end: usable or EDS_ERR_NOT_USABLE); an all-zero system (x = 0 by the zero-pivot rule); a window without points"""
    out = wsh.run_standalone(list(wsc.cases().values()))
    m = re.search(r"winsolve standalone: (\d+) cases; (\d+) solves, (\d+) usable, (\d+) not usable, (\d+) refused, (\d+) state errors, "
                  r"(\d+) marginalisations, (\d+) energies", out)
    assert m, out
    n_cases, solves, usable, not_usable, refused, state, margs, energies = (int(v) for v in m.groups())
    assert n_cases == len(wsc.cases()) and margs == n_cases and energies > 8 * n_cases
    assert solves > 40 * n_cases and usable >= 7 * n_cases and not_usable > 0 and refused > 7 * n_cases and state >= n_cases - 1
