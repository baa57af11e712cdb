"""include/eds_hip_epiline.h, the epiline tracker's companion header: plain C like eds_hip.h, its border numbers are OpenCV's, and every
function it declares is exported by libeds_hip.so and bound in capi.EPI_EXPORTS (no GPU needed: nothing here launches anything)."""
import header_checks as hc

capi = hc.capi


def test_epiline_header_is_c99_and_cxx11_clean(tmp_path):
    hc.compiles_clean("eds_hip_epiline.h", "EDS_EPI_BORDER_REFLECT_101 == 4 ? 0 : 1", tmp_path)


def test_epiline_declarations_equal_binding():
    # cv::BORDER_CONSTANT, REPLICATE, REFLECT, REFLECT_101 (= BORDER_DEFAULT)
    assert (capi.EPI_BORDER_CONSTANT, capi.EPI_BORDER_REPLICATE, capi.EPI_BORDER_REFLECT, capi.EPI_BORDER_REFLECT_101) == (0, 1, 2, 4)


def test_epiline_c_program_links_every_declared_function(tmp_path):
    hc.link_and_run("eds_hip_epiline.h", hc.declared("eds_hip_epiline.h"), [
        "    if (eds_epi_abi_version() != EDS_HIP_EPILINE_ABI_VERSION || EDS_HIP_EPILINE_ABI_VERSION != 1) return 3;",
        "    if (EDS_EPI_BORDER_CONSTANT != 0 || EDS_EPI_BORDER_REPLICATE != 1 || EDS_EPI_BORDER_REFLECT != 2) return 4;",
        "    if (eds_epi_track_points(0, 0, 1, 7, 4, 0, 1, 0, 0, 0, 0, 0, 0, 0) != EDS_ERR_INVALID) return 5;",
        "    if (eds_epi_get(0, 0, 0) != EDS_ERR_INVALID || eds_epi_get_model(0, 0, 0) != EDS_ERR_INVALID) return 6;",
        "    if (eds_epi_depth_update(0, 0, 1, 0, 0, 0) != EDS_ERR_INVALID) return 7;"], tmp_path)


def test_epiline_header_is_a_build_input():
    """a header-only edit must rebuild the library (capi.build's staleness check)"""
    assert hc.is_build_input("eds_hip_epiline.h") and hc.is_build_input("eds_epiline.hip")
    assert hc.contraction_off(hc.compile_line("eds_epiline.o"))
