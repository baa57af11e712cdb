"""The tracker handle's memory has one owner: no file of csrc/ calls the runtime's allocation functions itself but the owner,
the caller-owned eds_dev_malloc / eds_dev_free of eds_ingest.hip and the other library's eds_gather.hip; the per-module free functions
and the forks they made necessary are gone; and eds_trk holds its owner by value (no GPU needed: the sources are only read)."""
import os

import header_checks as hc

capi = hc.capi

RAW_CALLS = ("hipMalloc(", "hipFree(", "hipHostMalloc(", "hipHostFree(", "hipHostGetDevicePointer(")
MAY_CALL_THEM = {"eds_device_owner.hpp", "eds_ingest.hip", "eds_gather.hip"}
GONE = ("eds_fused_free", "eds_frame_free", "eds_points_free", "eds_depth_free", "eds_klt_free", "eds_epi_free", "eds_kfp_free", "eds_kfs_free",
        "eds_keyframe_free", "eds_strips_free", "device_alloc", "stage_is_ours")


def _sources():
    names = sorted(f for f in os.listdir(capi.CSRC) if f.endswith((".hip", ".hpp")))
    assert len(names) > 60 and MAY_CALL_THEM <= set(names)
    return {f: open(os.path.join(capi.CSRC, f)).read() for f in names}


def test_only_the_owner_calls_the_allocation_functions():
    found = [(f, call) for f, text in _sources().items() if f not in MAY_CALL_THEM for call in RAW_CALLS if call in text]
    assert not found, found
    owner = _sources()["eds_device_owner.hpp"]
    assert all(call in owner for call in RAW_CALLS)


def test_the_free_functions_and_their_forks_are_gone():
    texts = {f: open(os.path.join(capi.CSRC, f), errors="ignore").read() for f in sorted(os.listdir(capi.CSRC)) if os.path.isfile(os.path.join(capi.CSRC, f))
             and not f.endswith((".so", ".o"))}
    found = [(f, name) for f, text in texts.items() for name in GONE if name in text]
    assert not found, found


def test_the_tracker_holds_its_owner_by_value():
    handle = _sources()["eds_handle.hpp"]
    assert "edscapi::DeviceOwner own;" in handle
    assert "hipStream_t st =" not in handle and " dev = 0" not in handle           # one copy of the stream and the device: the owner's
    assert hc.is_build_input("eds_device_owner.hpp") and hc.is_build_input("eds_handle.hpp")
