"""include/eds_hip_kfswitch.h, the companion header of the batched keyframe switch: plain C like eds_hip.h, and every function it
declares is exported by libeds_hip.so and bound in capi.KFS_EXPORTS (no GPU needed: nothing here launches anything)."""
import importlib
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "eds_hip_kfswitch.h")
capi = importlib.import_module("slam-eds_amd.capi")


def _declared_functions():
    text = re.sub(r"/\*.*?\*/", " ", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(eds_kfs_[a-z0-9_]+)\s*\(", text)))


def test_kfswitch_header_is_c99_and_cxx11_clean(tmp_path):
    for std, cc, ext in (("-std=c99", "gcc", "c"), ("-std=c++11", "g++", "cpp")):
        src = tmp_path / ("inc." + ext)
        src.write_text('#include "eds_hip_kfswitch.h"\nint main(void) { return EDS_HIP_KFSWITCH_ABI_VERSION == 1 ? 0 : 1; }\n')
        subprocess.check_call([cc, std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                               "-o", str(tmp_path / "inc.o")])


def test_kfswitch_declarations_equal_binding():
    assert _declared_functions() == sorted(capi.KFS_EXPORTS)
    others = (set(capi.EXPORTS) | set(capi.DEPTH_EXPORTS) | set(capi.KLT_EXPORTS) | set(capi.EPI_EXPORTS) | set(capi.DEV_EXPORTS) |
              set(capi.KFP_EXPORTS))
    assert not set(capi.KFS_EXPORTS) & others


def test_kfswitch_c_program_links_every_declared_function(tmp_path):
    capi.build()
    names = _declared_functions()
    lines = ['#include <stdio.h>', '#include "eds_hip_kfswitch.h"', '#include "eds_hip_kfpoints.h"', "int main(void) {", "    const void* f[] = {"]
    lines += [f"        (const void*)(size_t)&{n}," for n in names]
    lines += ["    };", "    size_t i, n = sizeof(f) / sizeof(f[0]);", "    int m = 1;", "    int32_t perm = 0;", "    double xy[2] = {0, 0};",
              "    const void* img = xy;", "    eds_kf_select sel;", "    eds_kfs_depth d;", "    eds_kfs_out o;",
              "    for (i = 0; i < n; ++i) if (!f[i]) return 2;",
              "    if (eds_kfs_abi_version() != EDS_HIP_KFSWITCH_ABI_VERSION || EDS_HIP_KFSWITCH_ABI_VERSION != 1) return 3;",
              "    if (eds_abi_version() != 6 || eds_kfp_abi_version() != 1) return 4;",
              "    if (eds_kfs_tree_capacity() < 4096 || eds_kfs_chunk_size() < 1) return 5;",
              "    eds_kf_select_default(&sel);", "    d.source = EDS_KFS_DEPTH_NONE; o.n_points = 0;",
              "    if (eds_kfs_build_tree(0, 1, &m, xy, 1, &perm, 0) != EDS_ERR_INVALID) return 6;",
              "    if (eds_kfs_build_keyframes(0, 0, 1, EDS_IMG_F64, &img, &sel, xy, &d, &o) != EDS_ERR_INVALID) return 7;",
              "    if (eds_kfs_build_keyframes_dev(0, 0, 1, EDS_IMG_F64, img, 0, 0, &sel, xy, &d, &o) != EDS_ERR_INVALID) return 8;",
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


def test_kfswitch_sources_are_build_inputs():
    """a header-only edit must rebuild the library (capi.build's staleness check); the switch runs the keyframe build's fp64 kernels, so
    it is built without FMA contraction; the shared headers are prerequisites of every object"""
    import inspect
    assert "eds_hip_kfswitch.h" in inspect.getsource(capi.build)
    mk = open(os.path.join(capi.CSRC, "Makefile")).read()
    for f in ("eds_kfswitch.hip", "eds_hip_kfswitch.h", "eds_kfswitch.hpp", "eds_kdbuild.hpp", "eds_keyframe_kernels.hpp"):
        assert f in mk, f
    assert "eds_kfswitch.o: HIPFLAGS += -ffp-contract=off" in mk


def test_ctypes_structs_match_the_header(tmp_path):
    """sizeof and the offset of the last member of eds_kfs_depth / eds_kfs_out as the C compiler lays them out"""
    import ctypes as C
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "eds_hip_kfswitch.h"\nint main(void) { printf("%d %d %d %d\\n", (int)sizeof(eds_kfs_depth), '
                   '(int)offsetof(eds_kfs_depth, K_dst), (int)sizeof(eds_kfs_out), (int)offsetof(eds_kfs_out, weights)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(capi.KfsDepth), capi.KfsDepth.K_dst.offset, C.sizeof(capi.KfsOut), capi.KfsOut.weights.offset]
