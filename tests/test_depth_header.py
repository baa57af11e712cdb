"""include/eds_hip_depth.h, the inverse-depth filter's companion header: plain C like eds_hip.h, every function it declares is
exported by libeds_hip.so and bound in capi.DEPTH_EXPORTS (no GPU needed: nothing here launches anything)."""
import header_checks as hc

capi = hc.capi


def test_depth_c_program_links_every_declared_function(tmp_path):
    hc.link_and_run("eds_hip_depth.h", hc.declared("eds_hip_depth.h"), [
        "    eds_depth_params prm;",
        "    if (eds_depth_abi_version() != EDS_HIP_DEPTH_ABI_VERSION) return 3;",
        "    eds_depth_params_default(&prm);",
        "    if (prm.threshold != 100.0 || prm.init_a != 2.0 || prm.init_b != 5.0) return 4;",
        "    if (sizeof(eds_depth_summary) != 24) return 5;"], tmp_path)


def test_depth_header_is_a_build_input():
    """a header-only edit must rebuild the library (capi.build's staleness check)"""
    assert hc.is_build_input("eds_hip_depth.h") and hc.is_build_input("eds_depth.hip")
