"""include/eds_hip_winflag.h, the companion header of the points' residual history: plain C like eds_hip.h, every function it declares
is exported by libeds_hip.so and listed in capi.WFL_EXPORTS, every entry point answers a NULL handle with EDS_ERR_INVALID, its sources
are build inputs, the other window headers declare what they declared before; and the stand-alone program of csrc/eds_winflag.hpp
under g++ (tests/winflag_harness.py) over made-up windows and hostile values (no GPU needed: nothing here launches anything)."""
import importlib
import os
import re

import winflag_harness as wfh
import header_checks as hc

capi = hc.capi
winflag = importlib.import_module("slam-eds_amd.winflag")


def test_winflag_header_is_c99_and_cxx11_clean(tmp_path):
    hc.compiles_clean("eds_hip_winflag.h", "EDS_HIP_WINFLAG_ABI_VERSION == 1 && EDS_HIP_WINEDIT_ABI_VERSION == 1 ? 0 : 1", tmp_path)


def test_winflag_declarations_equal_binding():
    for name, exports in (("eds_hip_window.h", capi.WIN_EXPORTS), ("eds_hip_winsolve.h", capi.WSV_EXPORTS), ("eds_hip_winedit.h", capi.WED_EXPORTS)):
        assert hc.declared(name) == sorted(exports)
    text = open(os.path.join(capi.INCLUDE, "eds_hip_winflag.h")).read()
    for phrase in ("numGoodResiduals", "lastResiduals", "END of the point's run", "relBS = (float)(0.01 * (double)sqrtf(dx * dx + dy * dy))", "a NaN never wins",
                   "testing [0] first", "clear_is_new", "EDS_ERR_STATE", "HessianBlocks.h:474-497", "resetOOB", "only_empty", "not recomputed",
                   "size - visInToMarg < min_good_active_res_for_marg"):
        assert phrase in text, phrase
    body = re.search(r"typedef struct eds_wfl_history \{(.*?)\} eds_wfl_history;", re.sub(r"/\*.*?\*/", " ", text, flags=re.S), flags=re.S).group(1)
    assert re.findall(r"\*\s*([a-zA-Z_]+);", body) == [k for k, _, _ in winflag.HISTORY_FIELDS] == [k for k, _ in winflag.History._fields_]


def test_winflag_c_program_links_every_declared_function(tmp_path):
    hc.link_and_run("eds_hip_winflag.h", hc.declared("eds_hip_winflag.h"), [
        "    eds_wfl_history h = {0, 0, 0, 0, 0}; int32_t m[8] = {0, 0, 0, 0, 0, 0, 0, 0}; float p[108];",
        "    for (i = 0; i < 108; ++i) p[i] = 0.0f;",
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
        "      if (EDS_WFL_KEEP != 0 || EDS_WFL_MARGINALIZE != 1 || EDS_WFL_DROP != 2) return 12; }"], tmp_path)


def test_winflag_sources_are_build_inputs():
    for f in ("eds_winflag.hip", "eds_hip_winflag.h", "eds_winflag.hpp", "eds_dso_common.hpp"):
        assert hc.is_build_input(f), f
    assert hc.contraction_off(hc.compile_line("eds_winflag.o")) and hc.contraction_off(hc.resources_line("eds_winflag.hip"))
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
