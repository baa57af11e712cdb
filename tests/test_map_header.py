"""include/eds_hip_map.h, the header of the map's clouds and depth maps: plain C like eds_hip.h, every function it declares is exported
by libeds_hip.so and listed in capi.MAP_EXPORTS, every entry point answers a NULL handle with EDS_ERR_INVALID, every Python wrapper of
slam-eds_amd.map exists, and its sources are build inputs (no GPU needed: nothing here launches anything)."""
import importlib
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "eds_hip_map.h")
capi = importlib.import_module("slam-eds_amd.capi")


def _declared_functions():
    text = re.sub(r"/\*.*?\*/", " ", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(eds_map_[a-z0-9_A-Z]+)\s*\(", text)))


def test_map_header_is_c99_and_cxx11_clean(tmp_path):
    for std, cc, ext in (("-std=c99", "gcc", "c"), ("-std=c++11", "g++", "cpp")):
        src = tmp_path / ("inc." + ext)
        src.write_text('#include "eds_hip_map.h"\n#include "eds_hip_kfswitch.h"\n'
                       "int main(void) { return EDS_HIP_MAP_ABI_VERSION == 1 && EDS_MAP_FAN == 8 && EDS_MAP_MAX_IMM_HOSTS == 32 ? 0 : 1; }\n")
        subprocess.check_call([cc, std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                               "-o", str(tmp_path / "inc.o")])


def test_map_declarations_equal_binding():
    assert _declared_functions() == sorted(capi.MAP_EXPORTS)
    others = (set(capi.EXPORTS) | set(capi.DEPTH_EXPORTS) | set(capi.KLT_EXPORTS) | set(capi.EPI_EXPORTS) | set(capi.DEV_EXPORTS) |
              set(capi.KFP_EXPORTS) | set(capi.KFS_EXPORTS) | set(capi.IMM_EXPORTS) | set(capi.CT_EXPORTS) | set(capi.WIN_EXPORTS) |
              set(capi.WSV_EXPORTS) | set(capi.WED_EXPORTS) | set(capi.WFL_EXPORTS) | set(capi.ACT_EXPORTS) | set(capi.SEL_EXPORTS) |
              set(capi.INI_EXPORTS) | set(capi.UND_EXPORTS))
    assert not set(capi.MAP_EXPORTS) & others
    assert len(set(capi.MAP_EXPORTS)) == len(capi.MAP_EXPORTS)


def test_map_c_program_links_every_declared_function(tmp_path):
    capi.build()
    names = _declared_functions()
    lines = ['#include <stdio.h>', '#include "eds_hip_map.h"', "int main(void) {", "    const void* f[] = {"]
    lines += [f"        (const void*)(size_t)&{n}," for n in names]
    lines += ["    };", "    size_t i, n = sizeof(f) / sizeof(f[0]);",
              "    double T[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, K[4] = {1, 1, 0, 0}, out[8] = {0}; float cal[4] = {1, 1, 0, 0}, x = 0;",
              "    int32_t m = 7, s = 0; int k = 7; uint8_t b = 0;",
              "    for (i = 0; i < n; ++i) if (!f[i]) return 2;",
              "    if (eds_map_abi_version() != EDS_HIP_MAP_ABI_VERSION || EDS_HIP_MAP_ABI_VERSION != 1) return 3;",
              "    if (eds_abi_version() != 6 || eds_win_abi_version() != 1 || eds_imm_abi_version() != 1) return 4;",
              "    if (eds_map_window_cloud(0, 2, 3u, T, 1, out, 0, &m, 0) != EDS_ERR_INVALID || m != 7) return 5;",
              "    if (eds_map_window_depth_maps(0, 2, 3u, T, 1, T, K, 8, 8, 1, out, out, &s, 0, &m) != EDS_ERR_INVALID || m != 7) return 6;",
              "    if (eds_map_immature_cloud(0, 1, 1u, T, cal, 1, 1, out, out, &b, 0, &m) != EDS_ERR_INVALID || m != 7) return 7;",
              "    if (eds_map_set_immature_trace(0, 0, &x, &x, &s) != EDS_ERR_INVALID) return 8;",
              "    if (eds_map_slot_cloud(0, 0, 1, T, 1, out, 0, &k) != EDS_ERR_INVALID || k != 7) return 9;",
              "    for (i = 0; i < 8; ++i) if (out[i] != 0) return 10;",
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
    assert "eds_hip_map.h" in inspect.getsource(capi.build)
    mk = open(os.path.join(capi.CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    hdrs = re.search(r"^HDRS\s*:=(.*)$", mk, re.M).group(1).split()
    assert "eds_map.hip" in srcs
    assert "eds_map.hpp" in hdrs and "eds_map_internal.hpp" in hdrs and "../../include/eds_hip_map.h" in hdrs and "eds_dso_common.hpp" in hdrs
    assert "eds_map.o: HIPFLAGS += -ffp-contract=off" in mk
    assert "-c eds_map.hip -o /dev/null" in mk
