"""include/eds_hip_device.h, the companion header for inputs that already live in device memory: plain C like eds_hip.h, its own ABI
version, and every function it declares is exported by libeds_hip.so and bound in capi.DEV_EXPORTS (no GPU needed: nothing here
launches anything)."""
import header_checks as hc

capi = hc.capi
ALL_HEADERS = ("eds_hip.h", "eds_hip_depth.h", "eds_hip_klt.h", "eds_hip_epiline.h", "eds_hip_device.h")


def test_device_declarations_equal_binding():
    assert all(n.startswith("eds_dev_") for n in hc.declared("eds_hip_device.h"))


def test_all_five_headers_compile_as_c99_and_cxx11(tmp_path):
    hc.compiles_clean(ALL_HEADERS, "EDS_HIP_DEVICE_ABI_VERSION == 1 && EDS_HIP_ABI_VERSION == 6 ? 0 : 1", tmp_path)


def test_device_c_program_links_every_declared_function(tmp_path):
    """links against the library and calls what needs neither a handle nor a device: the version, and the argument checks that
    return before anything touches the HIP runtime"""
    hc.link_and_run(ALL_HEADERS, hc.declared("eds_hip_device.h"), [
        "    if (eds_dev_abi_version() != EDS_HIP_DEVICE_ABI_VERSION || EDS_HIP_DEVICE_ABI_VERSION != 1) return 3;",
        "    if (eds_abi_version() != 6) return 4;",
        "    if (eds_dev_set_event_frames(0, 0, 1, EDS_IMG_F32, 0, 0, 0) != EDS_ERR_INVALID) return 5;",
        "    if (eds_dev_set_keyframes(0, 0, 1, 0, 0, 0, 0, 0, 0, 0) != EDS_ERR_INVALID) return 6;",
        "    if (eds_dev_set_idepths(0, 0, 1, 0, 0, 1) != EDS_ERR_INVALID) return 7;",
        "    if (eds_dev_build_event_frames(0, 0, 1, 0, 0, 0, 0, 0, 0.5, 1, 0) != EDS_ERR_INVALID) return 8;",
        "    if (eds_dev_wait_stream(0, 0) != EDS_ERR_INVALID || eds_dev_signal_stream(0, 0) != EDS_ERR_INVALID) return 9;",
        "    if (eds_dev_malloc(0, 16, 0) != EDS_ERR_INVALID || eds_dev_upload(0, 0, 4) != EDS_ERR_INVALID) return 10;"], tmp_path)


def test_device_header_is_a_build_input():
    """a header-only edit must rebuild the library (capi.build's staleness check), and the ingest kernels are compiled without
    contraction: u0 = fx x + cx has to round as the host build rounds it"""
    assert hc.is_build_input("eds_hip_device.h") and hc.is_build_input("eds_ingest.hip")
    assert hc.contraction_off(hc.compile_line("eds_ingest.o"))


def test_other_abi_tuples_are_untouched():
    assert len(capi.EXPORTS) == len(set(capi.EXPORTS)) and "eds_trk_set_event_frames" in capi.EXPORTS
    assert not any(n.startswith("eds_dev_") for n in capi.EXPORTS + capi.DEPTH_EXPORTS + capi.KLT_EXPORTS + capi.EPI_EXPORTS)
