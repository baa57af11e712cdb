"""include/eds_hip_device.h, the companion header for inputs that already live in device memory: plain C like eds_hip.h, its own ABI
version, and every function it declares is exported by libeds_hip.so and bound in capi.DEV_EXPORTS (no GPU needed: nothing here
launches anything)."""
import importlib
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "eds_hip_device.h")
ALL_HEADERS = ("eds_hip.h", "eds_hip_depth.h", "eds_hip_klt.h", "eds_hip_epiline.h", "eds_hip_device.h")
capi = importlib.import_module("slam-eds_amd.capi")


def _declared_functions():
    text = re.sub(r"/\*.*?\*/", " ", open(HDR).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(eds_[a-z0-9_]+)\s*\(", text)))


def test_device_declarations_equal_binding():
    names = _declared_functions()
    assert names == sorted(capi.DEV_EXPORTS)
    assert all(n.startswith("eds_dev_") for n in names)
    others = set(capi.EXPORTS) | set(capi.DEPTH_EXPORTS) | set(capi.KLT_EXPORTS) | set(capi.EPI_EXPORTS)
    assert not set(capi.DEV_EXPORTS) & others
    assert len(set(capi.DEV_EXPORTS)) == len(capi.DEV_EXPORTS)


def test_all_five_headers_compile_as_c99_and_cxx11(tmp_path):
    body = "".join(f'#include "{h}"\n' for h in ALL_HEADERS)
    body += "int main(void) { return EDS_HIP_DEVICE_ABI_VERSION == 1 && EDS_HIP_ABI_VERSION == 6 ? 0 : 1; }\n"
    for std, cc, ext in (("-std=c99", "gcc", "c"), ("-std=c++11", "g++", "cpp")):
        src = tmp_path / ("inc." + ext)
        src.write_text(body)
        subprocess.check_call([cc, std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                               "-o", str(tmp_path / "inc.o")])


def test_device_c_program_links_every_declared_function(tmp_path):
    """links against the library and calls what needs neither a handle nor a device: the version, and the argument checks that
    return before anything touches the HIP runtime"""
    capi.build()
    names = _declared_functions()
    lines = ["#include <stdio.h>"] + [f'#include "{h}"' for h in ALL_HEADERS] + ["int main(void) {", "    const void* f[] = {"]
    lines += [f"        (const void*)(size_t)&{n}," for n in names]
    lines += ["    };", "    size_t i, n = sizeof(f) / sizeof(f[0]);",
              "    for (i = 0; i < n; ++i) if (!f[i]) return 2;",
              "    if (eds_dev_abi_version() != EDS_HIP_DEVICE_ABI_VERSION || EDS_HIP_DEVICE_ABI_VERSION != 1) return 3;",
              "    if (eds_abi_version() != 6) return 4;",
              "    if (eds_dev_set_event_frames(0, 0, 1, EDS_IMG_F32, 0, 0, 0) != EDS_ERR_INVALID) return 5;",
              "    if (eds_dev_set_keyframes(0, 0, 1, 0, 0, 0, 0, 0, 0, 0) != EDS_ERR_INVALID) return 6;",
              "    if (eds_dev_set_idepths(0, 0, 1, 0, 0, 1) != EDS_ERR_INVALID) return 7;",
              "    if (eds_dev_build_event_frames(0, 0, 1, 0, 0, 0, 0, 0, 0.5, 1, 0) != EDS_ERR_INVALID) return 8;",
              "    if (eds_dev_wait_stream(0, 0) != EDS_ERR_INVALID || eds_dev_signal_stream(0, 0) != EDS_ERR_INVALID) return 9;",
              "    if (eds_dev_malloc(0, 16, 0) != EDS_ERR_INVALID || eds_dev_upload(0, 0, 4) != EDS_ERR_INVALID) return 10;",
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


def test_device_header_is_a_build_input():
    """a header-only edit must rebuild the library (capi.build's staleness check), and the ingest kernels are compiled without
    contraction: u0 = fx x + cx has to round as the host build rounds it"""
    import inspect
    assert "eds_hip_device.h" in inspect.getsource(capi.build)
    mk = open(os.path.join(capi.CSRC, "Makefile")).read()
    assert "eds_ingest.hip" in mk and "eds_hip_device.h" in mk and "eds_ingest.o: HIPFLAGS += -ffp-contract=off" in mk


def test_other_abi_tuples_are_untouched():
    assert len(capi.EXPORTS) == len(set(capi.EXPORTS)) and "eds_trk_set_event_frames" in capi.EXPORTS
    assert not any(n.startswith("eds_dev_") for n in capi.EXPORTS + capi.DEPTH_EXPORTS + capi.KLT_EXPORTS + capi.EPI_EXPORTS)
