"""include/eds_hip_depth.h, the inverse-depth filter's companion header: plain C like eds_hip.h, every function it declares is
exported by libeds_hip.so and bound in capi.DEPTH_EXPORTS (no GPU needed: nothing here launches anything)."""
import importlib
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "eds_hip_depth.h")
capi = importlib.import_module("slam-eds_amd.capi")


def _declared_functions():
    text = re.sub(r"/\*.*?\*/", " ", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(eds_[a-z0-9_]+)\s*\(", text)))


def test_depth_header_is_c99_and_cxx11_clean(tmp_path):
    for std, cc, ext in (("-std=c99", "gcc", "c"), ("-std=c++11", "g++", "cpp")):
        src = tmp_path / ("inc." + ext)
        src.write_text('#include "eds_hip_depth.h"\nint main(void) { return 0; }\n')
        subprocess.check_call([cc, std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                               "-o", str(tmp_path / "inc.o")])


def test_depth_declarations_equal_binding():
    assert _declared_functions() == sorted(capi.DEPTH_EXPORTS)
    assert not set(capi.DEPTH_EXPORTS) & set(capi.EXPORTS)


def test_depth_c_program_links_every_declared_function(tmp_path):
    capi.build()
    names = _declared_functions()
    lines = ['#include <stdio.h>', '#include "eds_hip_depth.h"', "int main(void) {", "    const void* f[] = {"]
    lines += [f"        (const void*)(size_t)&{n}," for n in names]
    lines += ["    };", "    size_t i, n = sizeof(f) / sizeof(f[0]);", "    eds_depth_params prm;",
              "    for (i = 0; i < n; ++i) if (!f[i]) return 2;",
              "    if (eds_depth_abi_version() != EDS_HIP_DEPTH_ABI_VERSION) return 3;",
              "    eds_depth_params_default(&prm);",
              "    if (prm.threshold != 100.0 || prm.init_a != 2.0 || prm.init_b != 5.0) return 4;",
              "    if (sizeof(eds_depth_summary) != 24) return 5;",
              '    printf("%d functions\\n", (int)n);', "    return 0;", "}"]
    src = tmp_path / "link.c"
    src.write_text("\n".join(lines) + "\n")
    libdir = os.path.dirname(capi.LIB_PATH)
    exe = tmp_path / "link"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-leds_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    assert f"{len(names)} functions" in subprocess.check_output([str(exe)], text=True)


def test_depth_header_is_a_build_input():
    """a header-only edit must rebuild the library (capi.build's staleness check)"""
    import inspect
    assert "eds_hip_depth.h" in inspect.getsource(capi.build)
    mk = open(os.path.join(capi.CSRC, "Makefile")).read()
    assert "eds_depth.hip" in mk and "eds_hip_depth.h" in mk
