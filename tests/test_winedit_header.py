"""include/eds_hip_winedit.h, the companion header of the window's table edits: plain C like eds_hip.h, every function it declares is
exported by libeds_hip.so and listed in capi.WED_EXPORTS, every entry point answers a NULL handle with EDS_ERR_INVALID, its sources are
build inputs, the two window headers declare what they declared before; and the stand-alone program of csrc/eds_winedit.hpp under g++
(tests/winedit_harness.py) over the cases and the hostile flags (no GPU needed: nothing here launches anything)."""
import importlib
import os
import re

import winedit_harness as weh
import winsolve_cases as wsc
import header_checks as hc

capi = hc.capi
winedit = importlib.import_module("slam-eds_amd.winedit")


def test_winedit_header_is_c99_and_cxx11_clean(tmp_path):
    hc.compiles_clean("eds_hip_winedit.h", "EDS_HIP_WINEDIT_ABI_VERSION == 1 && EDS_HIP_WINSOLVE_ABI_VERSION == 1 ? 0 : 1", tmp_path)


def test_winedit_declarations_equal_binding():
    # the two window headers declare exactly what they declared: nothing of this header leaked into them
    for name, exports in (("eds_hip_window.h", capi.WIN_EXPORTS), ("eds_hip_winsolve.h", capi.WSV_EXPORTS)):
        assert hc.declared(name) == sorted(exports)
    # the header says what it must: the stable order, and that the swap-with-back is not restated
    text = open(os.path.join(capi.INCLUDE, "eds_hip_winedit.h")).read()
    assert "STABLE" in text and "swap-with-back" in text and "NOT restated" in text
    # ... and every step of marginalizeFrame's arithmetic, the stated inverse and its tie rule included
    for phrase in ("sqrt(|H_ii| + 10)", "exact no-ops", "partial pivoting", "LOWEST r on", "ONE subtraction", "0.5 * (H_ij + H_ji)", "EDS_ERR_NOT_USABLE"):
        assert phrase in text, phrase


def test_winedit_c_program_links_every_declared_function(tmp_path):
    hc.link_and_run("eds_hip_winedit.h", hc.declared("eds_hip_winedit.h"), [
        "    eds_wed_out out; int32_t m[8] = {0, 0, 0, 0, 0, 0, 0, 0};",
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
        "    if (sizeof(eds_wed_out) != 10 * sizeof(void*)) return 9;"], tmp_path)


def test_winedit_binding_matches_the_harness():
    assert [k for k, _, _ in winedit.OUT_FIELDS] == [k for k, _, _ in weh.OUT_FIELDS] == [k for k, _ in winedit.Out._fields_]
    assert winedit.STATE_FIELDS == weh.STATE_FIELDS
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(capi.INCLUDE, "eds_hip_winedit.h")).read(), flags=re.S)
    body = re.search(r"typedef struct eds_wed_out \{(.*?)\} eds_wed_out;", text, flags=re.S).group(1)
    assert re.findall(r"\*\s*([a-zA-Z_]+);", body) == [k for k, _, _ in winedit.OUT_FIELDS]
    for method in ("remove_residuals", "remove_points", "marginalize_frame", "insert_activated", "set_state", "counts", "rows"):
        assert callable(getattr(winedit.WindowEdit, method)) and callable(getattr(weh.HostEdit, method))


def test_winedit_sources_are_build_inputs():
    for f in ("eds_winedit.hip", "eds_hip_winedit.h", "eds_winedit.hpp", "eds_window_internal.hpp", "eds_device_owner.hpp", "eds_dso_common.hpp"):
        assert hc.is_build_input(f), f
    assert hc.contraction_off(hc.compile_line("eds_winedit.o")) and hc.contraction_off(hc.resources_line("eds_winedit.hip"))
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
