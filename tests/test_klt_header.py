"""include/eds_hip_klt.h, the KLT point trackers' companion header: plain C like eds_hip.h, its ABI version is the library's, and every
function it declares is exported by libeds_hip.so and bound in capi.KLT_EXPORTS (no GPU needed: nothing here launches anything)."""
import header_checks as hc

capi = hc.capi
HEADERS = ("eds_hip_klt.h", "eds_hip_depth.h")


def test_klt_header_is_c99_and_cxx11_clean(tmp_path):
    hc.compiles_clean(HEADERS, "EDS_DEPTH_DEVICE_TRACKS == 3 ? 0 : 1", tmp_path)


def test_klt_declarations_equal_binding():
    assert capi.DEPTH_DEVICE_TRACKS == 3


def test_klt_c_program_links_every_declared_function(tmp_path):
    hc.link_and_run(HEADERS, hc.declared("eds_hip_klt.h"), [
        "    if (eds_klt_abi_version() != EDS_HIP_KLT_ABI_VERSION || EDS_HIP_KLT_ABI_VERSION != 1) return 3;",
        "    if (eds_depth_abi_version() != EDS_HIP_DEPTH_ABI_VERSION || EDS_HIP_DEPTH_ABI_VERSION != 2) return 4;",
        "    if (eds_klt_track_points(0, 0, 1, 7, 0, 0, 0, 0, 0, 0) != EDS_ERR_INVALID) return 5;",
        "    if (eds_klt_get(0, 0, 0, 0) != EDS_ERR_INVALID) return 6;"], tmp_path)


def test_klt_header_is_a_build_input():
    """a header-only edit must rebuild the library (capi.build's staleness check)"""
    assert hc.is_build_input("eds_hip_klt.h") and hc.is_build_input("eds_klt.hip")
    assert hc.contraction_off(hc.compile_line("eds_klt.o"))
