"""include/eds_hip_winflag.h, the companion header of the points' residual history: plain C like eds_hip.h, every function it declares
is exported by libeds_hip.so and listed in capi.WFL_EXPORTS, every entry point answers a NULL handle with EDS_ERR_INVALID, its sources
are build inputs, the other window headers declare what they declared before; and the stand-alone program of csrc/eds_winflag.hpp
under g++ (tests/winflag_harness.py) over made-up windows and hostile values (no GPU needed: nothing here launches anything)."""
import importlib
import inspect
import os
import re
import subprocess

import winflag_harness as wfh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "eds_hip_winflag.h")
capi = importlib.import_module("slam-eds_amd.capi")
winflag = importlib.import_module("slam-eds_amd.winflag")


def _declared(path, prefix):
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(" + prefix + r"[a-z0-9_]+)\s*\(", text)))


def test_winflag_header_is_c99_and_cxx11_clean(tmp_path):
    for std, cc_, ext in (("-std=c99", "gcc", "c"), ("-std=c++11", "g++", "cpp")):
        src = tmp_path / ("inc." + ext)
        src.write_text('#include "eds_hip_winflag.h"\nint main(void) { return EDS_HIP_WINFLAG_ABI_VERSION == 1 && EDS_HIP_WINEDIT_ABI_VERSION == 1 ? 0 : 1; }\n')
        subprocess.check_call([cc_, std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                               "-o", str(tmp_path / "inc.o")])


def test_winflag_declarations_equal_binding():
    assert _declared(HDR, "eds_wfl_") == sorted(capi.WFL_EXPORTS)
    others = (set(capi.EXPORTS) | set(capi.DEV_EXPORTS) | set(capi.IMM_EXPORTS) | set(capi.WIN_EXPORTS) | set(capi.WSV_EXPORTS) | set(capi.WED_EXPORTS) |
              set(capi.ACT_EXPORTS) | set(capi.SEL_EXPORTS))
    assert not set(capi.WFL_EXPORTS) & others and len(set(capi.WFL_EXPORTS)) == len(capi.WFL_EXPORTS)
    for name, prefix, exports in (("eds_hip_window.h", "eds_win_", capi.WIN_EXPORTS), ("eds_hip_winsolve.h", "eds_wsv_", capi.WSV_EXPORTS),
                                  ("eds_hip_winedit.h", "eds_wed_", capi.WED_EXPORTS)):
        path = os.path.join(ROOT, "include", name)
        assert _declared(path, prefix) == sorted(exports)
        assert not _declared(path, "eds_wfl_")
    text = open(HDR).read()
    for phrase in ("numGoodResiduals", "lastResiduals", "END of the point's run", "relBS = (float)(0.01 * (double)sqrtf(dx * dx + dy * dy))", "a NaN never wins",
                   "testing [0] first", "clear_is_new", "EDS_ERR_STATE", "HessianBlocks.h:474-497", "resetOOB", "only_empty", "not recomputed",
                   "size - visInToMarg < min_good_active_res_for_marg"):
        assert phrase in text, phrase
    body = re.search(r"typedef struct eds_wfl_history \{(.*?)\} eds_wfl_history;", re.sub(r"/\*.*?\*/", " ", text, flags=re.S), flags=re.S).group(1)
    assert re.findall(r"\*\s*([a-zA-Z_]+);", body) == [k for k, _, _ in winflag.HISTORY_FIELDS] == [k for k, _ in winflag.History._fields_]


def test_winflag_c_program_links_every_declared_function(tmp_path):
    capi.build()
    names = _declared(HDR, "eds_wfl_")
    lines = ['#include <stdio.h>', '#include "eds_hip_winflag.h"', "int main(void) {", "    const void* f[] = {"]
    lines += [f"        (const void*)(size_t)&{n}," for n in names]
    lines += ["    };", "    size_t i, n = sizeof(f) / sizeof(f[0]);", "    eds_wfl_history h = {0, 0, 0, 0, 0}; int32_t m[8] = {0, 0, 0, 0, 0, 0, 0, 0}; float p[108];",
              "    for (i = 0; i < 108; ++i) p[i] = 0.0f;",
              "    for (i = 0; i < n; ++i) if (!f[i]) return 2;",
              "    if (eds_wfl_abi_version() != EDS_HIP_WINFLAG_ABI_VERSION || EDS_HIP_WINFLAG_ABI_VERSION != 1) return 3;",
              "    if (eds_win_abi_version() != 1 || eds_wsv_abi_version() != 1 || eds_wed_abi_version() != 1) return 4;",
              "    if (eds_wfl_set_history(0, &h, 0) != EDS_ERR_INVALID || eds_wfl_get_history(0, &h) != EDS_ERR_INVALID) return 5;",
              "    if (eds_wfl_insert_frame_residuals(0, 0, m) != EDS_ERR_INVALID) return 6;",
              "    if (eds_wfl_apply_fixed(0, 2, p, 0, m) != EDS_ERR_INVALID) return 7;",
              "    if (sizeof(eds_wfl_history) != 5 * sizeof(void*)) return 8;",
              "    { eds_wfl_params q; double d[8] = {0, 0, 0, 0, 0, 0, 0, 0};",
              "      eds_wfl_params_default(&q); eds_wfl_params_default(0);",
              "      if (q.min_good_active_res_for_marg != 3 || q.min_good_res_for_marg != 4 || q.min_idepth_h_marg != 50.0f || sizeof(q) != 16) return 9;",
              "      if (eds_wfl_flag_points(0, 2, 0u, &q, p, p, 0, m) != EDS_ERR_INVALID || eds_wfl_get_fates(0, m) != EDS_ERR_INVALID) return 10;",
              "      if (eds_wfl_marginalize_flagged(0, 1.0f, 1.0, d, d, m) != EDS_ERR_INVALID || eds_wfl_remove_flagged(0, m, m) != EDS_ERR_INVALID) return 11;",
              "      if (EDS_WFL_KEEP != 0 || EDS_WFL_MARGINALIZE != 1 || EDS_WFL_DROP != 2) return 12; }",
              '    printf("%d functions\\n", (int)n);', "    return 0;", "}"]
    src = tmp_path / "link.c"
    src.write_text("\n".join(lines) + "\n")
    libdir = os.path.dirname(capi.LIB_PATH)
    exe = tmp_path / "link"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-leds_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    assert f"{len(names)} functions" in subprocess.check_output([str(exe)], text=True)
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    assert set(names) <= set(re.findall(r"\s[TW]\s+(\S+)", out))


def test_winflag_sources_are_build_inputs():
    assert "eds_hip_winflag.h" in inspect.getsource(capi.build)
    mk = open(os.path.join(capi.CSRC, "Makefile")).read()
    for f in ("eds_winflag.hip", "eds_hip_winflag.h", "eds_winflag.hpp", "eds_dso_common.hpp"):
        assert f in mk, f
    assert "eds_winflag.o: HIPFLAGS += -ffp-contract=off" in mk
    assert "-ffp-contract=off -Rpass-analysis=kernel-resource-usage -c eds_winflag.hip" in mk
    text = open(os.path.join(capi.CSRC, "eds_winflag.hip")).read()
    assert '#include "eds_window_internal.hpp"' in text and '#include "eds_winflag.hpp"' in text and "struct eds_win {" not in text
    # every atomic adds an integer count (of states, of fates); no float is summed across lanes
    atomics = [line for line in text.splitlines() if "atomicAdd(" in line]
    assert len(atomics) == 3 and all("atomicAdd(counts + " in line for line in atomics)
    # the edits carry the columns along, and only once they exist
    edit = open(os.path.join(capi.CSRC, "eds_winedit.hip")).read()
    assert '#include "eds_winflag.hpp"' in edit and edit.count("h->wfl") >= 5
    for method in ("set_history", "history", "insert_frame_residuals", "apply_fixed", "flag_points", "fates", "marginalize_flagged", "remove_flagged"):
        assert callable(getattr(winflag.WindowFlags, method))


def test_standalone_program_builds_and_survives_the_hostile_values():
    """the program of the sanitizer run, built plainly: windows of 2 .. 8 frames, an empty one and one of up to 3 000 points
    among them, with NaN, infinities, zeros and denormals in the precalc records, the inverse depths and the maxima; the pass, a
    removal, every frame's insert within and beyond the capacity, a frame's removal, activated points"""
    out = wfh.run_standalone()
    m = re.search(r"winflag standalone: (\d+) windows; (\d+) passes, (\d+) residuals inserted, (\d+) forgotten, (\d+) refused, (\d+) flaggings", out)
    assert m, out
    windows, passes, inserted, forgotten, refused, flaggings = (int(v) for v in m.groups())
    assert windows == passes == 7 * 6 and inserted > 1000 and forgotten > 1000 and refused >= 7 * 5 and flaggings >= 4 * windows
