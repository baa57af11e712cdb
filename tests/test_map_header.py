"""include/eds_hip_map.h, the header of the map's clouds and depth maps: plain C like eds_hip.h, every function it declares is exported
by libeds_hip.so and listed in capi.MAP_EXPORTS, every entry point answers a NULL handle with EDS_ERR_INVALID, every Python wrapper of
slam-eds_amd.map exists, and its sources are build inputs (no GPU needed: nothing here launches anything)."""
import importlib
import inspect
import os
import re

import header_checks as hc

capi = hc.capi


def test_map_header_is_c99_and_cxx11_clean(tmp_path):
    hc.compiles_clean(("eds_hip_map.h", "eds_hip_kfswitch.h"),
                      "EDS_HIP_MAP_ABI_VERSION == 1 && EDS_MAP_FAN == 8 && EDS_MAP_MAX_IMM_HOSTS == 32 ? 0 : 1", tmp_path)


def test_map_c_program_links_every_declared_function(tmp_path):
    hc.link_and_run("eds_hip_map.h", hc.declared("eds_hip_map.h"), [
        "    double T[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, K[4] = {1, 1, 0, 0}, out[8] = {0}; float cal[4] = {1, 1, 0, 0}, x = 0;",
        "    int32_t m = 7, s = 0; int k = 7; uint8_t b = 0;",
        "    if (eds_map_abi_version() != EDS_HIP_MAP_ABI_VERSION || EDS_HIP_MAP_ABI_VERSION != 1) return 3;",
        "    if (eds_abi_version() != 6 || eds_win_abi_version() != 1 || eds_imm_abi_version() != 1) return 4;",
        "    if (eds_map_window_cloud(0, 2, 3u, T, 1, out, 0, &m, 0) != EDS_ERR_INVALID || m != 7) return 5;",
        "    if (eds_map_window_depth_maps(0, 2, 3u, T, 1, T, K, 8, 8, 1, out, out, &s, 0, &m) != EDS_ERR_INVALID || m != 7) return 6;",
        "    if (eds_map_immature_cloud(0, 1, 1u, T, cal, 1, 1, out, out, &b, 0, &m) != EDS_ERR_INVALID || m != 7) return 7;",
        "    if (eds_map_set_immature_trace(0, 0, &x, &x, &s) != EDS_ERR_INVALID) return 8;",
        "    if (eds_map_slot_cloud(0, 0, 1, T, 1, out, 0, &k) != EDS_ERR_INVALID || k != 7) return 9;",
        "    for (i = 0; i < 8; ++i) if (out[i] != 0) return 10;"], tmp_path)


def test_every_python_wrapper_exists():
    mp = importlib.import_module("slam-eds_amd.map")
    for name in ("window_cloud", "window_depth_maps", "immature_cloud", "slot_cloud", "set_immature_trace", "build_keyframes_from_window"):
        assert callable(getattr(mp, name)), name
    assert "device" in inspect.signature(mp.window_cloud).parameters and "device" in inspect.signature(mp.window_depth_maps).parameters
    assert "device" in inspect.signature(mp.immature_cloud).parameters and "device" in inspect.signature(mp.slot_cloud).parameters
    assert mp._lib().eds_map_abi_version() == 1
    import np_map_oracle as mo
    assert mp.FAN == len(mo.FAN) == 8 and [tuple(c) for c in mo.COLORS.tolist()] == list(mp.STATUS_COLORS)


def test_the_shared_header_and_the_library_agree_on_the_sweep():
    """tests/map_cases.py sizes its cases by edsmap::CHUNK; the kernels' workgroup is that constant"""
    import map_harness as mh
    src = open(os.path.join(capi.CSRC, "eds_map.hip")).read()
    assert "constexpr int CT = edsmap::CHUNK;" in src and "__launch_bounds__(CT) void k_map_depth" in src
    assert mh.chunk() == int(re.search(r"constexpr int CHUNK = (\d+);", open(os.path.join(capi.CSRC, "eds_map.hpp")).read()).group(1))


def test_map_sources_are_build_inputs():
    """a header-only edit must rebuild the library (capi.build's staleness check); getMap's mixed-width arithmetic is restated without
    FMA contraction; the shared headers are prerequisites of every object"""
    for f in ("eds_map.hip", "eds_hip_map.h", "eds_map.hpp", "eds_map_internal.hpp", "eds_dso_common.hpp"):
        assert hc.is_build_input(f), f
    assert hc.contraction_off(hc.compile_line("eds_map.o")) and hc.resources_line("eds_map.hip")
