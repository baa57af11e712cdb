"""include/eds_hip_immdepth.h, the header of the depth-seeded immature points: plain C like eds_hip.h, ABI version 1, every function it
declares is exported by libeds_hip.so and listed in capi.IMD_EXPORTS and bound in slam-eds_amd.immdepth, every entry point answers a NULL
handle with EDS_ERR_INVALID, and its sources are build inputs (no GPU needed: nothing here launches anything)."""
import ctypes as C
import importlib
import inspect
import os

import header_checks as hc

capi = hc.capi


def test_immdepth_header_is_c99_and_cxx11_clean(tmp_path):
    hc.compiles_clean(("eds_hip_immdepth.h", "eds_hip_select.h", "eds_hip_map.h"),
                      "EDS_HIP_IMMDEPTH_ABI_VERSION == 1 && EDS_IMD_WALK_GLOBAL == 1 && sizeof(eds_imd_info) == 32 ? 0 : 1", tmp_path)


def test_immdepth_c_program_links_every_declared_function(tmp_path):
    hc.link_and_run("eds_hip_immdepth.h", hc.declared("eds_hip_immdepth.h"), [
        "    double xy[2] = {1, 2}, idp[1] = {1}, sc[2] = {1, 1}, dist = 7; float t[1] = {1}, fi = 7; int32_t uv[2] = {9, 9}, cnt[2] = {7, 7}, idx = 7;",
        "    int k = 7; uint8_t b = 7; eds_imd_info info;",
        "    if (eds_imd_abi_version() != EDS_HIP_IMMDEPTH_ABI_VERSION || EDS_HIP_IMMDEPTH_ABI_VERSION != 1) return 3;",
        "    if (eds_abi_version() != 6 || eds_imm_abi_version() != 1) return 4;",
        "    if (eds_imd_set_depth_map(0, 1, xy, idp, 0, &k) != EDS_ERR_INVALID || k != 7) return 5;",
        "    if (eds_imd_create_points_selected(0, 0, 0, 3, 3, 9, 9, sc, &b, &k, cnt) != EDS_ERR_INVALID || k != 7 || b != 7 || cnt[0] != 7) return 6;",
        "    if (eds_imd_create_points(0, 0, 1, uv, t, 0, sc, &b, cnt) != EDS_ERR_INVALID || b != 7 || cnt[1] != 7) return 7;",
        "    if (eds_imd_get_nearest(0, 0, &idx, &fi, &dist) != EDS_ERR_INVALID || idx != 7 || fi != 7 || dist != 7) return 8;",
        "    if (eds_imd_get_tree(0, &idx, xy, idp) != EDS_ERR_INVALID || idx != 7) return 9;",
        "    if (eds_imd_set_debug(0, 0) != EDS_ERR_INVALID || eds_imd_get_info(0, &info) != EDS_ERR_INVALID) return 10;"], tmp_path)


def test_every_python_wrapper_exists_and_the_record_matches():
    idp = importlib.import_module("slam-eds_amd.immdepth")
    mp = importlib.import_module("slam-eds_amd.map")
    for name in ("set_depth_map", "create_points_selected", "create_points", "nearest", "tree", "set_debug", "info"):
        assert callable(getattr(idp.ImmatureDepth, name)), name
    assert callable(mp.seed_immature_from_window) and "rect" in inspect.signature(mp.seed_immature_from_window).parameters
    assert "scale" in inspect.signature(idp.ImmatureDepth.create_points).parameters
    L = idp._lib()
    assert L.eds_imd_abi_version() == 1
    assert all(getattr(L, n).argtypes is not None for n in capi.IMD_EXPORTS if n != "eds_imd_abi_version")
    assert C.sizeof(idp.Info) == 32 and idp.Info.nn_kernel_ms.offset == 24
    assert idp.WALK_GLOBAL == 1


def test_other_headers_keep_their_abi_numbers():
    L = capi.lib()
    assert (L.eds_abi_version(), L.eds_imm_abi_version(), L.eds_kfs_abi_version(), L.eds_map_abi_version(), L.eds_sel_abi_version()) == (6, 1, 1, 1, 1)


def test_immdepth_sources_are_build_inputs():
    """a header-only edit must rebuild the library (capi.build's staleness check); the loop's fp64 arithmetic is restated without FMA
    contraction; k_kd_build lives in one shared header that both of its translation units include"""
    for f in ("eds_immdepth.hip", "eds_hip_immdepth.h", "eds_immdepth.hpp", "eds_kdbuild_kernel.hpp"):
        assert hc.is_build_input(f), f
    assert hc.contraction_off(hc.compile_line("eds_immdepth.o")) and hc.contraction_off(hc.resources_line("eds_immdepth.hip"))
    for f in ("eds_kfswitch.hip", "eds_immdepth.hip"):
        text = open(os.path.join(capi.CSRC, f)).read()
        assert '#include "eds_kdbuild_kernel.hpp"' in text and "void k_kd_build(" not in text, f
    assert open(os.path.join(capi.CSRC, "eds_kdbuild_kernel.hpp")).read().count("void k_kd_build(") == 1
