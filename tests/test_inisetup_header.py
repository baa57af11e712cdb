"""include/eds_hip_inisetup.h, the companion header of the rest of setFirst: plain C like eds_hip_init.h, every function it declares is
exported by libeds_hip.so, listed in capi.INISETUP_EXPORTS and bound in slam-eds_amd/init.py, its ABI version function agrees with the
macro, eds_hip_init.h's ABI stays 1, and every call refuses its arguments before it touches the device (no GPU needed: nothing here
launches anything)."""
import importlib
import os

import header_checks as hc

capi = hc.capi
init = importlib.import_module("slam-eds_amd.init")


def test_inisetup_header_is_c99_and_cxx11_clean(tmp_path):
    hc.compiles_clean("eds_hip_inisetup.h", "EDS_HIP_INISETUP_ABI_VERSION == 1 && EDS_HIP_INIT_ABI_VERSION == 1 ? 0 : 1", tmp_path)


def test_inisetup_declarations_equal_binding():
    capi.build()
    L = init._lib()
    for name in hc.declared("eds_hip_inisetup.h"):
        assert getattr(L, name).argtypes is not None, name
    assert L.eds_ini_setup_abi_version() == 1 and L.eds_ini_abi_version() == 1
    for method in ("sparsity", "make_pixel_status", "pixel_status", "set_points_status", "make_neighbours", "neighbours", "setup_levels"):
        assert hasattr(init.CoarseInitializer, method), method


def test_inisetup_c_program_links_every_function_and_arguments_are_refused_before_the_device(tmp_path):
    hc.link_and_run("eds_hip_inisetup.h", hc.declared("eds_hip_inisetup.h"), [
        "    int32_t m = 0, k = 0, nb[20], par[2]; uint8_t b = 0; float x = 0;",
        "    if (eds_ini_setup_abi_version() != EDS_HIP_INISETUP_ABI_VERSION || EDS_HIP_INISETUP_ABI_VERSION != 1) return 3;",
        "    if (eds_ini_abi_version() != 1 || EDS_INI_SPARSITY_START != 5 || EDS_INI_NN_TILE < 64) return 4;",
        "    if (eds_ini_get_sparsity(0, &m) != EDS_ERR_INVALID || eds_ini_set_sparsity(0, 3) != EDS_ERR_INVALID) return 5;",
        "    if (eds_ini_make_pixel_status(0, 1, 100.f, 5, 1.f, &m, &k) != EDS_ERR_INVALID) return 6;",
        "    if (eds_ini_get_pixel_status(0, 1, &b) != EDS_ERR_INVALID || eds_ini_set_points_status(0, 1, &m) != EDS_ERR_INVALID) return 7;",
        "    if (eds_ini_make_neighbours(0, 0) != EDS_ERR_INVALID || eds_ini_get_neighbours(0, 0, nb, par) != EDS_ERR_INVALID) return 8;",
        "    if (eds_ini_get_neighbours_kernel_ms(0, &x) != EDS_ERR_INVALID || eds_ini_setup_levels(0, 0, 0, &m) != EDS_ERR_INVALID) return 9;"], tmp_path)


def test_inisetup_sources_are_build_inputs():
    for f in ("eds_inisetup.hip", "eds_hip_inisetup.h", "eds_inisetup.hpp", "eds_init_internal.hpp", "eds_dso_common.hpp"):
        assert hc.is_build_input(f), f
    assert hc.contraction_off(hc.compile_line("eds_inisetup.o")) and hc.contraction_off(hc.resources_line("eds_inisetup.hip"))
    hip = open(os.path.join(capi.CSRC, "eds_inisetup.hip")).read()
    assert "hipMalloc" not in hip and "hipFree" not in hip and "own.alloc(" in hip
    # every launch and every wait of the file is counted on the handle, as eds_init.hip's are
    assert hip.count("hipLaunchKernelGGL(") == 1 and "++(h)->n_launches;" in hip
    assert hip.count("edscapi::read_back(") == 1 and hip.count("++h->n_waits;") == 1
    for other in ("hipStreamSynchronize", "hipDeviceSynchronize", "hipEventSynchronize", "hipMemcpy(", "hipMemset(", "<<<"):
        assert other not in hip, other
