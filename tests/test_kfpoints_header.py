"""include/eds_hip_kfpoints.h, the companion header of the keyframe's own point set: plain C like eds_hip.h, and every function it declares
is exported by libeds_hip.so and bound in capi.KFP_EXPORTS (no GPU needed: nothing here launches anything)."""
import header_checks as hc


def test_kfpoints_c_program_links_every_declared_function(tmp_path):
    hc.link_and_run("eds_hip_kfpoints.h", hc.declared("eds_hip_kfpoints.h"), [
        "    uint8_t flag = 1;", "    int k = 0;",
        "    if (eds_kfp_abi_version() != EDS_HIP_KFPOINTS_ABI_VERSION || EDS_HIP_KFPOINTS_ABI_VERSION != 1) return 3;",
        "    if (eds_abi_version() != 6) return 4;",
        "    if (eds_kfp_refine_points(0, 0, 1, 1.0, 11, 4, 255, 1, 0, 0, 0, 0) != EDS_ERR_INVALID) return 5;",
        "    if (eds_kfp_clean_points(0, 0, 1, 0.2, 0, 0, 0) != EDS_ERR_INVALID) return 6;",
        "    if (eds_kfp_erase_points(0, 0, 1, 1, &flag, 0, 0) != EDS_ERR_INVALID) return 7;",
        "    if (eds_kfp_counts(0, 0, 1, &k, &k) != EDS_ERR_INVALID) return 8;",
        "    if (eds_kfp_project_depth_map(0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0) != EDS_ERR_INVALID) return 9;"], tmp_path)


def test_kfpoints_header_and_flag_are_build_inputs():
    """a header-only edit must rebuild the library (capi.build's staleness check), and the projection is built without FMA contraction"""
    for f in ("eds_kfpoints.hip", "eds_hip_kfpoints.h", "eds_kfpoints.hpp"):
        assert hc.is_build_input(f), f
    assert hc.contraction_off(hc.compile_line("eds_kfpoints.o"))
