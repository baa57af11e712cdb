"""include/eds_hip_inisetup.h, the companion header of the rest of setFirst: plain C like eds_hip_init.h, every function it declares is
exported by libeds_hip.so, listed in capi.INISETUP_EXPORTS and bound in slam-eds_amd/init.py, its ABI version function agrees with the
macro, eds_hip_init.h's ABI stays 1, and every call refuses its arguments before it touches the device (no GPU needed: nothing here
launches anything)."""
import importlib
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "eds_hip_inisetup.h")
capi = importlib.import_module("slam-eds_amd.capi")
init = importlib.import_module("slam-eds_amd.init")


def _declared_functions():
    text = re.sub(r"/\*.*?\*/", " ", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(eds_ini_[a-z0-9_]+)\s*\(", text)))


def test_inisetup_header_is_c99_and_cxx11_clean(tmp_path):
    for std, cc_, ext in (("-std=c99", "gcc", "c"), ("-std=c++11", "g++", "cpp")):
        src = tmp_path / ("inc." + ext)
        src.write_text('#include "eds_hip_inisetup.h"\nint main(void) { return EDS_HIP_INISETUP_ABI_VERSION == 1 && EDS_HIP_INIT_ABI_VERSION == 1 ? 0 : 1; }\n')
        subprocess.check_call([cc_, std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                               "-o", str(tmp_path / "inc.o")])


def test_inisetup_declarations_equal_binding():
    names = _declared_functions()
    assert names == sorted(capi.INISETUP_EXPORTS) and len(set(capi.INISETUP_EXPORTS)) == len(capi.INISETUP_EXPORTS)
    assert not set(capi.INISETUP_EXPORTS) & set(capi.INI_EXPORTS)
    capi.build()
    L = init._lib()
    for name in names:
        assert getattr(L, name).argtypes is not None, name
    assert L.eds_ini_setup_abi_version() == 1 and L.eds_ini_abi_version() == 1
    for method in ("sparsity", "make_pixel_status", "pixel_status", "set_points_status", "make_neighbours", "neighbours", "setup_levels"):
        assert hasattr(init.CoarseInitializer, method), method


def test_inisetup_c_program_links_every_function_and_arguments_are_refused_before_the_device(tmp_path):
    capi.build()
    names = _declared_functions()
    lines = ['#include <stdio.h>', '#include "eds_hip_inisetup.h"', "int main(void) {", "    const void* f[] = {"]
    lines += [f"        (const void*)(size_t)&{n}," for n in names]
    lines += ["    };", "    size_t i, n = sizeof(f) / sizeof(f[0]);", "    int32_t m = 0, k = 0, nb[20], par[2]; uint8_t b = 0; float x = 0;",
              "    for (i = 0; i < n; ++i) if (!f[i]) return 2;",
              "    if (eds_ini_setup_abi_version() != EDS_HIP_INISETUP_ABI_VERSION || EDS_HIP_INISETUP_ABI_VERSION != 1) return 3;",
              "    if (eds_ini_abi_version() != 1 || EDS_INI_SPARSITY_START != 5 || EDS_INI_NN_TILE < 64) return 4;",
              "    if (eds_ini_get_sparsity(0, &m) != EDS_ERR_INVALID || eds_ini_set_sparsity(0, 3) != EDS_ERR_INVALID) return 5;",
              "    if (eds_ini_make_pixel_status(0, 1, 100.f, 5, 1.f, &m, &k) != EDS_ERR_INVALID) return 6;",
              "    if (eds_ini_get_pixel_status(0, 1, &b) != EDS_ERR_INVALID || eds_ini_set_points_status(0, 1, &m) != EDS_ERR_INVALID) return 7;",
              "    if (eds_ini_make_neighbours(0, 0) != EDS_ERR_INVALID || eds_ini_get_neighbours(0, 0, nb, par) != EDS_ERR_INVALID) return 8;",
              "    if (eds_ini_get_neighbours_kernel_ms(0, &x) != EDS_ERR_INVALID || eds_ini_setup_levels(0, 0, 0, &m) != EDS_ERR_INVALID) return 9;",
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


def test_inisetup_sources_are_build_inputs():
    import inspect
    assert "eds_hip_inisetup.h" in inspect.getsource(capi.build)
    mk = open(os.path.join(capi.CSRC, "Makefile")).read()
    for f in ("eds_inisetup.hip", "eds_hip_inisetup.h", "eds_inisetup.hpp", "eds_init_internal.hpp", "eds_dso_common.hpp"):
        assert f in mk, f
    assert "eds_inisetup.o: HIPFLAGS += -ffp-contract=off" in mk
    assert "-ffp-contract=off -Rpass-analysis=kernel-resource-usage -c eds_inisetup.hip" in mk
    hip = open(os.path.join(capi.CSRC, "eds_inisetup.hip")).read()
    assert "hipMalloc" not in hip and "hipFree" not in hip and "own.alloc(" in hip
    # every launch and every wait of the file is counted on the handle, as eds_init.hip's are
    assert hip.count("hipLaunchKernelGGL(") == 1 and "++(h)->n_launches;" in hip
    assert hip.count("edscapi::read_back(") == 1 and hip.count("++h->n_waits;") == 1
    for other in ("hipStreamSynchronize", "hipDeviceSynchronize", "hipEventSynchronize", "hipMemcpy(", "hipMemset(", "<<<"):
        assert other not in hip, other
