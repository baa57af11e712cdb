"""include/eds_hip_winedit.h, the companion header of the window's table edits: plain C like eds_hip.h, every function it declares is
exported by libeds_hip.so and listed in capi.WED_EXPORTS, every entry point answers a NULL handle with EDS_ERR_INVALID, its sources are
build inputs, the two window headers declare what they declared before; and the stand-alone program of csrc/eds_winedit.hpp under g++
(tests/winedit_harness.py) over the cases and the hostile flags (no GPU needed: nothing here launches anything)."""
import importlib
import os
import re
import subprocess

import winedit_harness as weh
import winsolve_cases as wsc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "eds_hip_winedit.h")
capi = importlib.import_module("slam-eds_amd.capi")
winedit = importlib.import_module("slam-eds_amd.winedit")


def _declared(path, prefix):
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(" + prefix + r"[a-z0-9_]+)\s*\(", text)))


def test_winedit_header_is_c99_and_cxx11_clean(tmp_path):
    for std, cc_, ext in (("-std=c99", "gcc", "c"), ("-std=c++11", "g++", "cpp")):
        src = tmp_path / ("inc." + ext)
        src.write_text('#include "eds_hip_winedit.h"\nint main(void) { return EDS_HIP_WINEDIT_ABI_VERSION == 1 && EDS_HIP_WINSOLVE_ABI_VERSION == 1 ? 0 : 1; }\n')
        subprocess.check_call([cc_, std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                               "-o", str(tmp_path / "inc.o")])


def test_winedit_declarations_equal_binding():
    assert _declared(HDR, "eds_wed_") == sorted(capi.WED_EXPORTS)
    others = (set(capi.EXPORTS) | set(capi.DEPTH_EXPORTS) | set(capi.KLT_EXPORTS) | set(capi.EPI_EXPORTS) | set(capi.DEV_EXPORTS) |
              set(capi.KFP_EXPORTS) | set(capi.KFS_EXPORTS) | set(capi.IMM_EXPORTS) | set(capi.CT_EXPORTS) | set(capi.WIN_EXPORTS) |
              set(capi.WSV_EXPORTS) | set(capi.ACT_EXPORTS) | set(capi.SEL_EXPORTS))
    assert not set(capi.WED_EXPORTS) & others
    assert len(set(capi.WED_EXPORTS)) == len(capi.WED_EXPORTS)
    # the two window headers declare exactly what they declared: nothing of this header leaked into them
    for name, prefix, exports in (("eds_hip_window.h", "eds_win_", capi.WIN_EXPORTS), ("eds_hip_winsolve.h", "eds_wsv_", capi.WSV_EXPORTS)):
        path = os.path.join(ROOT, "include", name)
        assert _declared(path, prefix) == sorted(exports)
        assert not _declared(path, "eds_wed_")
    # the header says what it must: the stable order, and that the swap-with-back is not restated
    text = open(HDR).read()
    assert "STABLE" in text and "swap-with-back" in text and "NOT restated" in text
    # ... and every step of marginalizeFrame's arithmetic, the stated inverse and its tie rule included
    for phrase in ("sqrt(|H_ii| + 10)", "exact no-ops", "partial pivoting", "LOWEST r on", "ONE subtraction", "0.5 * (H_ij + H_ji)", "EDS_ERR_NOT_USABLE"):
        assert phrase in text, phrase


def test_winedit_c_program_links_every_declared_function(tmp_path):
    capi.build()
    names = _declared(HDR, "eds_wed_")
    lines = ['#include <stdio.h>', '#include "eds_hip_winedit.h"', "int main(void) {", "    const void* f[] = {"]
    lines += [f"        (const void*)(size_t)&{n}," for n in names]
    lines += ["    };", "    size_t i, n = sizeof(f) / sizeof(f[0]);", "    eds_wed_out out; int32_t m[8] = {0, 0, 0, 0, 0, 0, 0, 0};",
              "    for (i = 0; i < n; ++i) if (!f[i]) return 2;",
              "    if (eds_wed_abi_version() != EDS_HIP_WINEDIT_ABI_VERSION || EDS_HIP_WINEDIT_ABI_VERSION != 1) return 3;",
              "    if (eds_abi_version() != 6 || eds_win_abi_version() != 1 || eds_wsv_abi_version() != 1) return 4;",
              "    if (eds_wed_remove_residuals(0, m, 0, m) != EDS_ERR_INVALID || eds_wed_remove_residuals(0, 0, 0, 0) != EDS_ERR_INVALID) return 5;",
              "    if (eds_wed_remove_points(0, m, 0, m, m) != EDS_ERR_INVALID) return 6;",
              "    if (eds_wed_counts(0, m, m, m) != EDS_ERR_INVALID) return 7;",
              "    { double d[8] = {0, 0, 0, 0, 0, 0, 0, 0};",
              "      if (eds_wed_marginalize_frame(0, 0, d, d, d, d, d, d) != EDS_ERR_INVALID) return 10;",
              "      if (eds_wed_set_state(0, 2, d, d, d, d, d, d, d) != EDS_ERR_INVALID) return 11; }",
              "    if (eds_wed_insert_activated(0, 0, m, m) != EDS_ERR_INVALID) return 12;",
              "    if (eds_wed_get(0, &out) != EDS_ERR_INVALID) return 8;",
              "    if (sizeof(eds_wed_out) != 10 * sizeof(void*)) return 9;",
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


def test_winedit_binding_matches_the_harness():
    assert [k for k, _, _ in winedit.OUT_FIELDS] == [k for k, _, _ in weh.OUT_FIELDS] == [k for k, _ in winedit.Out._fields_]
    assert winedit.STATE_FIELDS == weh.STATE_FIELDS
    text = re.sub(r"/\*.*?\*/", " ", open(HDR).read(), flags=re.S)
    body = re.search(r"typedef struct eds_wed_out \{(.*?)\} eds_wed_out;", text, flags=re.S).group(1)
    assert re.findall(r"\*\s*([a-zA-Z_]+);", body) == [k for k, _, _ in winedit.OUT_FIELDS]
    for method in ("remove_residuals", "remove_points", "marginalize_frame", "insert_activated", "set_state", "counts", "rows"):
        assert callable(getattr(winedit.WindowEdit, method)) and callable(getattr(weh.HostEdit, method))


def test_winedit_sources_are_build_inputs():
    import inspect
    assert "eds_hip_winedit.h" in inspect.getsource(capi.build)
    mk = open(os.path.join(capi.CSRC, "Makefile")).read()
    for f in ("eds_winedit.hip", "eds_hip_winedit.h", "eds_winedit.hpp", "eds_window_internal.hpp", "eds_device_owner.hpp", "eds_dso_common.hpp"):
        assert f in mk, f
    assert "eds_winedit.o: HIPFLAGS += -ffp-contract=off" in mk
    assert "-ffp-contract=off -Rpass-analysis=kernel-resource-usage -c eds_winedit.hip" in mk
    text = open(os.path.join(capi.CSRC, "eds_winedit.hip")).read()
    assert '#include "eds_window_internal.hpp"' in text and '#include "eds_winedit.hpp"' in text and "struct eds_win {" not in text
    # no sum of floats anywhere, so nothing to reorder: the kernels hold no floating-point atomic
    assert "atomic" not in text


def test_standalone_program_builds_and_survives_the_hostile_flags():
    """the program of the sanitizer run, built plainly: every case prepared with a state, a solve and a step, then six flag
    patterns (none, every third, first and last, one whole host, arbitrary nonzero words, all) through remove_residuals with a
    selection, remove_residuals(NULL), remove_points, another round of linearize -> solve -> step on what is left (the empty window
    included) and an edit without flags; then an edit before any eds_wsv state, and NULL flags; then every frame marginalised in turn
    until two are left, with eds_wed_set_state and a solve after each, and NaN / +-inf / 1e300 in HM, bM and the priors, a hosted
    point, an empty window (refused, not usable, or run to the end); and a made-up fit inserted: capacity exceeded by one point and by
    one residual (refused, nothing changes), an index outside the eds_imm, the insert itself, and an insert into an empty window"""
    out = weh.run_standalone(list(wsc.cases().values()))
    m = re.search(r"winedit standalone: (\d+) cases; (\d+) edits, (\d+) solves, (\d+) rows removed; (\d+) frames marginalised, (\d+) refused, (\d+) not usable", out)
    assert m, out
    n_cases, edits, solves, removed, frames, refused, not_usable = (int(v) for v in m.groups())
    assert n_cases == len(wsc.cases()) and edits == 25 * n_cases and solves >= 12 * n_cases and removed > 1000
    m2 = re.search(r"winedit standalone: (\d+) inserts, (\d+) refused for capacity", out)
    assert m2 and int(m2.group(1)) == 2 * n_cases and int(m2.group(2)) == 2 * n_cases, out
    assert frames == sum(s.F - 2 + 1 for s in wsc.cases().values() if s.F >= 3) and refused >= 8 * (n_cases - 1) and not_usable >= n_cases - 1
