"""include/eds_hip.h is the drop-in boundary: plain C.  It must compile as C99 and as C++11 with warnings as errors, a C program that
takes the address of EVERY function it declares must link against libeds_hip.so, and the struct sizes the C compiler sees must be the
ones the library was built with (no GPU needed: nothing here launches anything)."""
import header_checks as hc

capi = hc.capi


def test_header_is_c99_and_cxx11_clean(tmp_path):
    # both headers of the boundary: the tracker's C ABI and the RCCL gather of the result table (opaque pointers: no rccl.h needed to include it)
    hc.compiles_clean(("eds_hip.h", "eds_hip_rccl.h"), "0", tmp_path)


def test_c_program_links_every_declared_function(tmp_path):
    names = hc.declared("eds_hip.h")
    assert len(names) >= 50 and set(capi.EXPORTS) <= set(names), (len(names), sorted(set(capi.EXPORTS) - set(names)))
    hc.link_and_run("eds_hip.h", names, [
        "    if (eds_abi_version() != EDS_HIP_ABI_VERSION) return 3;",
        "    if (eds_trk_cfg_size() != (int)sizeof(eds_trk_cfg) || eds_trk_info_size() != (int)sizeof(eds_trk_info)) return 4;"], tmp_path)
