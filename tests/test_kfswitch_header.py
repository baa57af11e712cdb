"""include/eds_hip_kfswitch.h, the companion header of the batched keyframe switch: plain C like eds_hip.h, and every function it
declares is exported by libeds_hip.so and bound in capi.KFS_EXPORTS (no GPU needed: nothing here launches anything)."""
import ctypes as C
import subprocess

import header_checks as hc

capi = hc.capi


def test_kfswitch_c_program_links_every_declared_function(tmp_path):
    hc.link_and_run(("eds_hip_kfswitch.h", "eds_hip_kfpoints.h"), hc.declared("eds_hip_kfswitch.h"), [
        "    int m = 1;", "    int32_t perm = 0;", "    double xy[2] = {0, 0};",
        "    const void* img = xy;", "    eds_kf_select sel;", "    eds_kfs_depth d;", "    eds_kfs_out o;",
        "    if (eds_kfs_abi_version() != EDS_HIP_KFSWITCH_ABI_VERSION || EDS_HIP_KFSWITCH_ABI_VERSION != 1) return 3;",
        "    if (eds_abi_version() != 6 || eds_kfp_abi_version() != 1) return 4;",
        "    if (eds_kfs_tree_capacity() < 4096 || eds_kfs_chunk_size() < 1) return 5;",
        "    eds_kf_select_default(&sel);", "    d.source = EDS_KFS_DEPTH_NONE; o.n_points = 0;",
        "    if (eds_kfs_build_tree(0, 1, &m, xy, 1, &perm, 0) != EDS_ERR_INVALID) return 6;",
        "    if (eds_kfs_build_keyframes(0, 0, 1, EDS_IMG_F64, &img, &sel, xy, &d, &o) != EDS_ERR_INVALID) return 7;",
        "    if (eds_kfs_build_keyframes_dev(0, 0, 1, EDS_IMG_F64, img, 0, 0, &sel, xy, &d, &o) != EDS_ERR_INVALID) return 8;"], tmp_path)


def test_kfswitch_sources_are_build_inputs():
    """a header-only edit must rebuild the library (capi.build's staleness check); the switch runs the keyframe build's fp64 kernels, so
    it is built without FMA contraction; the shared headers are prerequisites of every object"""
    for f in ("eds_kfswitch.hip", "eds_hip_kfswitch.h", "eds_kfswitch.hpp", "eds_kdbuild.hpp", "eds_keyframe_kernels.hpp"):
        assert hc.is_build_input(f), f
    assert hc.contraction_off(hc.compile_line("eds_kfswitch.o"))


def test_ctypes_structs_match_the_header(tmp_path):
    """sizeof and the offset of the last member of eds_kfs_depth / eds_kfs_out as the C compiler lays them out"""
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "eds_hip_kfswitch.h"\nint main(void) { printf("%d %d %d %d\\n", (int)sizeof(eds_kfs_depth), '
                   '(int)offsetof(eds_kfs_depth, K_dst), (int)sizeof(eds_kfs_out), (int)offsetof(eds_kfs_out, weights)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", capi.INCLUDE, str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(capi.KfsDepth), capi.KfsDepth.K_dst.offset, C.sizeof(capi.KfsOut), capi.KfsOut.weights.offset]
