"""What is true of every public header (capi.HEADERS) and of every source of csrc/Makefile; the per-module tests keep what is theirs
(no GPU needed: nothing here launches anything)."""
import glob
import os

import pytest

import header_checks as hc

capi = hc.capi


@pytest.mark.parametrize("h", capi.HEADERS, ids=lambda h: h.file)
def test_header_is_plain_c_and_declares_exactly_its_table(h, tmp_path):
    hc.compiles_clean(h.file, f"{h.abi_macro} == {h.abi_version} ? 0 : 1", tmp_path)
    assert hc.declared(h.file) == sorted(h.exports)
    assert not set(h.exports) & hc.other_exports(h.exports)
    assert len(set(h.exports)) == len(h.exports)


def test_every_header_and_source_is_a_build_input():
    """a header-only edit must rebuild the library: every .hpp of csrc and every public header is a prerequisite of every object
    (HDRS) and is looked at by capi.build(); every .hip but the RCCL gather's, which is its own library, is a source (SRCS)"""
    csrc = lambda pattern: {os.path.basename(p) for p in glob.glob(os.path.join(capi.CSRC, pattern))}
    for name in sorted(csrc("*.hpp") | csrc("*.hip") - {"eds_gather.hip"} | {h.file for h in capi.HEADERS}):
        assert hc.is_build_input(name), name
    assert len(hc.make_variable("SRCS")) == len(set(hc.make_variable("SRCS"))) == len(csrc("*.hip")) - 1
    assert os.path.join(capi.CSRC, "eds_gather.hip") in capi.build_inputs() and "../../include/eds_hip_rccl.h" not in hc.make_variable("HDRS")


def test_resources_reports_every_source_with_its_objects_flags():
    for src in hc.make_variable("SRCS"):
        obj = hc.compile_line(src.replace(".hip", ".o"))
        assert hc.resources_line(src) == obj.replace(" -c ", " -Rpass-analysis=kernel-resource-usage -c ").rsplit(" -o ", 1)[0] + " -o /dev/null"
