"""include/eds_hip_immdepth.h, the header of the depth-seeded immature points: plain C like eds_hip.h, ABI version 1, every function it
declares is exported by libeds_hip.so and listed in capi.IMD_EXPORTS and bound in slam-eds_amd.immdepth, every entry point answers a NULL
handle with EDS_ERR_INVALID, and its sources are build inputs (no GPU needed: nothing here launches anything)."""
import ctypes as C
import importlib
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "eds_hip_immdepth.h")
capi = importlib.import_module("slam-eds_amd.capi")


def _declared_functions():
    text = re.sub(r"/\*.*?\*/", " ", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(eds_imd_[a-z0-9_]+)\s*\(", text)))


def test_immdepth_header_is_c99_and_cxx11_clean(tmp_path):
    for std, cc, ext in (("-std=c99", "gcc", "c"), ("-std=c++11", "g++", "cpp")):
        src = tmp_path / ("inc." + ext)
        src.write_text('#include "eds_hip_immdepth.h"\n#include "eds_hip_select.h"\n#include "eds_hip_map.h"\n'
                       "int main(void) { return EDS_HIP_IMMDEPTH_ABI_VERSION == 1 && EDS_IMD_WALK_GLOBAL == 1 && sizeof(eds_imd_info) == 32 ? 0 : 1; }\n")
        subprocess.check_call([cc, std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                               "-o", str(tmp_path / "inc.o")])


def test_immdepth_declarations_equal_binding():
    assert _declared_functions() == sorted(capi.IMD_EXPORTS)
    others = (set(capi.EXPORTS) | set(capi.DEPTH_EXPORTS) | set(capi.KLT_EXPORTS) | set(capi.EPI_EXPORTS) | set(capi.DEV_EXPORTS) |
              set(capi.KFP_EXPORTS) | set(capi.KFS_EXPORTS) | set(capi.IMM_EXPORTS) | set(capi.CT_EXPORTS) | set(capi.WIN_EXPORTS) |
              set(capi.WSV_EXPORTS) | set(capi.WED_EXPORTS) | set(capi.WFL_EXPORTS) | set(capi.ACT_EXPORTS) | set(capi.SEL_EXPORTS) |
              set(capi.INI_EXPORTS) | set(capi.UND_EXPORTS) | set(capi.MAP_EXPORTS))
    assert not set(capi.IMD_EXPORTS) & others
    assert len(set(capi.IMD_EXPORTS)) == len(capi.IMD_EXPORTS)


def test_immdepth_c_program_links_every_declared_function(tmp_path):
    capi.build()
    names = _declared_functions()
    lines = ['#include <stdio.h>', '#include "eds_hip_immdepth.h"', "int main(void) {", "    const void* f[] = {"]
    lines += [f"        (const void*)(size_t)&{n}," for n in names]
    lines += ["    };", "    size_t i, n = sizeof(f) / sizeof(f[0]);",
              "    double xy[2] = {1, 2}, idp[1] = {1}, sc[2] = {1, 1}, dist = 7; float t[1] = {1}, fi = 7; int32_t uv[2] = {9, 9}, cnt[2] = {7, 7}, idx = 7;",
              "    int k = 7; uint8_t b = 7; eds_imd_info info;",
              "    for (i = 0; i < n; ++i) if (!f[i]) return 2;",
              "    if (eds_imd_abi_version() != EDS_HIP_IMMDEPTH_ABI_VERSION || EDS_HIP_IMMDEPTH_ABI_VERSION != 1) return 3;",
              "    if (eds_abi_version() != 6 || eds_imm_abi_version() != 1) return 4;",
              "    if (eds_imd_set_depth_map(0, 1, xy, idp, 0, &k) != EDS_ERR_INVALID || k != 7) return 5;",
              "    if (eds_imd_create_points_selected(0, 0, 0, 3, 3, 9, 9, sc, &b, &k, cnt) != EDS_ERR_INVALID || k != 7 || b != 7 || cnt[0] != 7) return 6;",
              "    if (eds_imd_create_points(0, 0, 1, uv, t, 0, sc, &b, cnt) != EDS_ERR_INVALID || b != 7 || cnt[1] != 7) return 7;",
              "    if (eds_imd_get_nearest(0, 0, &idx, &fi, &dist) != EDS_ERR_INVALID || idx != 7 || fi != 7 || dist != 7) return 8;",
              "    if (eds_imd_get_tree(0, &idx, xy, idp) != EDS_ERR_INVALID || idx != 7) return 9;",
              "    if (eds_imd_set_debug(0, 0) != EDS_ERR_INVALID || eds_imd_get_info(0, &info) != EDS_ERR_INVALID) return 10;",
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
    assert "eds_hip_immdepth.h" in inspect.getsource(capi.build)
    mk = open(os.path.join(capi.CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    hdrs = re.search(r"^HDRS\s*:=(.*)$", mk, re.M).group(1).split()
    assert "eds_immdepth.hip" in srcs
    assert "eds_immdepth.hpp" in hdrs and "eds_kdbuild_kernel.hpp" in hdrs and "../../include/eds_hip_immdepth.h" in hdrs
    assert "eds_immdepth.o: HIPFLAGS += -ffp-contract=off" in mk
    assert "-ffp-contract=off -Rpass-analysis=kernel-resource-usage -c eds_immdepth.hip -o /dev/null" in mk
    for f in ("eds_kfswitch.hip", "eds_immdepth.hip"):
        text = open(os.path.join(capi.CSRC, f)).read()
        assert '#include "eds_kdbuild_kernel.hpp"' in text and "void k_kd_build(" not in text, f
    assert open(os.path.join(capi.CSRC, "eds_kdbuild_kernel.hpp")).read().count("void k_kd_build(") == 1
