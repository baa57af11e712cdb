"""include/eds_hip_klt.h, the KLT point trackers' companion header: plain C like eds_hip.h, its ABI version is the library's, and every
function it declares is exported by libeds_hip.so and bound in capi.KLT_EXPORTS (no GPU needed: nothing here launches anything)."""
import importlib
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "eds_hip_klt.h")
capi = importlib.import_module("slam-eds_amd.capi")


def _declared_functions():
    text = re.sub(r"/\*.*?\*/", " ", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(eds_[a-z0-9_]+)\s*\(", text)))


def test_klt_header_is_c99_and_cxx11_clean(tmp_path):
    for std, cc, ext in (("-std=c99", "gcc", "c"), ("-std=c++11", "g++", "cpp")):
        src = tmp_path / ("inc." + ext)
        src.write_text('#include "eds_hip_klt.h"\n#include "eds_hip_depth.h"\nint main(void) { return EDS_DEPTH_DEVICE_TRACKS == 3 ? 0 : 1; }\n')
        subprocess.check_call([cc, std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                               "-o", str(tmp_path / "inc.o")])


def test_klt_declarations_equal_binding():
    assert _declared_functions() == sorted(capi.KLT_EXPORTS)
    assert not set(capi.KLT_EXPORTS) & (set(capi.EXPORTS) | set(capi.DEPTH_EXPORTS))
    assert capi.DEPTH_DEVICE_TRACKS == 3


def test_klt_c_program_links_every_declared_function(tmp_path):
    capi.build()
    names = _declared_functions()
    lines = ['#include <stdio.h>', '#include "eds_hip_klt.h"', '#include "eds_hip_depth.h"', "int main(void) {", "    const void* f[] = {"]
    lines += [f"        (const void*)(size_t)&{n}," for n in names]
    lines += ["    };", "    size_t i, n = sizeof(f) / sizeof(f[0]);",
              "    for (i = 0; i < n; ++i) if (!f[i]) return 2;",
              "    if (eds_klt_abi_version() != EDS_HIP_KLT_ABI_VERSION || EDS_HIP_KLT_ABI_VERSION != 1) return 3;",
              "    if (eds_depth_abi_version() != EDS_HIP_DEPTH_ABI_VERSION || EDS_HIP_DEPTH_ABI_VERSION != 2) return 4;",
              "    if (eds_klt_track_points(0, 0, 1, 7, 0, 0, 0, 0, 0, 0) != EDS_ERR_INVALID) return 5;",
              "    if (eds_klt_get(0, 0, 0, 0) != EDS_ERR_INVALID) return 6;",
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


def test_klt_header_is_a_build_input():
    """a header-only edit must rebuild the library (capi.build's staleness check)"""
    import inspect
    assert "eds_hip_klt.h" in inspect.getsource(capi.build)
    mk = open(os.path.join(capi.CSRC, "Makefile")).read()
    assert "eds_klt.hip" in mk and "eds_hip_klt.h" in mk and "eds_klt.o: HIPFLAGS += -ffp-contract=off" in mk
